// Network-input ops of scannertools_caffe for gfx950: a decoded U8 RGB frame becomes a network's float32 input.
//
//   FacenetInput  /root/reference/scannertools_caffe/scannertools_caffe_cpp/facenet_input_kernel_cpu.cpp:81-117
//                 resize(INTER_LINEAR, to floor(size * scale) rounded up to a multiple of 8) -> convertTo(F32) ->
//                 subtract(mean_colors) -> split -> transpose x 3 -> plane copies: NINE passes in the reference, ONE
//                 kernel here (k_facenet_input).  The resize is cv::resize's 8-bit INTER_LINEAR (st_internal.h: the
//                 arithmetic of the Resize op, with its reroute to the exact 2 x 2 mean and the copy at equal size);
//                 parity is with the reference's CPU kernel (its CUDA twin resizes in float).
//   CaffeInput    .../caffe_input_kernel.cpp:75-138 + caffe_input_transformer_base.h:43-105 (a Halide pipeline): a
//                 separable box filter with half-pixel centres, horizontal pass first, clamp to 0..255, channel flip,
//                 mean subtraction, optional division by 255.  Window membership is computed on the HOST
//                 (st_caffe_input_axis) and handed to k_caffe_input as tables, so which pixels enter a mean never
//                 depends on device float division.
//
// Both kernels stage the source rows they need through LDS with 16-byte loads (a byte path serves frames or rows that
// are not 16-byte aligned) and are one launch per call (per 65 535 frames).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "st_internal.h"

// per-geometry plans of the two ops and the device buffer their tables live in (one per op and context)
struct st_netin_plan {
  int h = 0, w = 0, nh = 0, nw = 0;   // the geometry the plan is for; h == 0: none yet
  int status = ST_OK;                 // caffe: ST_ERR_UNSUPPORTED for a geometry with an empty window
  int mode = 0, cx = 0;               // facenet: RS_* path; both: output columns per workgroup
  int orows = 0, seg = 0, smax = 0;   // caffe: output rows per workgroup, bytes per staged row, rx rows
  size_t lds = 0;
  void* dev = nullptr;                // x table, then y table
  size_t dev_bytes = 0, y_off = 0;
};
struct st_netin_state {
  st_netin_plan facenet, caffe;
};

void st_netin_release(st_ctx* ctx) {
  if (!ctx->netin) return;
  if (ctx->netin->facenet.dev) (void)hipFree(ctx->netin->facenet.dev);
  if (ctx->netin->caffe.dev) (void)hipFree(ctx->netin->caffe.dev);
  delete ctx->netin;
  ctx->netin = nullptr;
}

namespace {

// ---- FacenetInput ---------------------------------------------------------------------------------
constexpr int FN_ROWS = 64;                 // output rows (y) of a tile: 16 lanes x 4 consecutive rows each
constexpr int FN_SEGD = 61;                 // dwords per staged row: 240 bytes + 1 dword, odd so that the 16 lanes of a column hit 16 banks
constexpr int FN_SEG_BYTES = 240;           // bytes of a source row a tile may need
constexpr int FN_MAX_CX = 64;               // output columns (x) of a tile

struct FnX { int sx; int a; };              // first tap's source column; 11-bit weights a0 | a1 << 16
struct FnY { int y0, y1, b0, b1; };         // the two source rows and their weights

struct FacenetK {
  const uint8_t* const* src;  // n RGB frames (sh, sw, 3)
  float* const* dst;          // n planar transposed (3, nw, nh) float frames
  const FnX* xt;              // nw entries
  const FnY* yt;              // nh entries
  int sh, sw, nh, nw, cx, mode;
  int vec_in, vec_out;        // every frame and source row 16-byte aligned; every output frame 16-byte aligned
  float mean[3];
};

// A tile is FN_ROWS output rows (y) x cx output columns (x).  The source rows the tile needs (two per output row: the
// taps of INTER_LINEAR, the pair of the 2 x 2 mean; one for a copy) are staged in LDS, restricted to the byte span the
// tile's columns read.  Then lanes run along y, the contiguous axis of the transposed output: thread (ly, lx) owns rows
// 4 ly .. 4 ly + 3 of columns lx, lx + 16, ...; its 4 floats per (channel, column) go out as one 16-byte store.
// Local row lr sits in slot (lr & 3) * 16 + (lr >> 2): the 16 lanes that read their j-th row together are FN_SEGD (odd)
// dwords apart and fall on 16 different banks.
__global__ __launch_bounds__(256) void k_facenet_input(FacenetK a) {
  __shared__ unsigned rows[2 * FN_ROWS * FN_SEGD];
  __shared__ FnX sxt[FN_MAX_CX];
  __shared__ FnY syt[FN_ROWS];
  const int t = threadIdx.x;
  const int x0 = blockIdx.x * a.cx, xe = min(x0 + a.cx, a.nw), ty0 = blockIdx.y * FN_ROWS;
  const uint8_t* __restrict__ src = st_gl(a.src[blockIdx.z]);
  const int extra = a.mode == RS_COPY ? 0 : 1;   // the second column a pixel reads
  // the tile's taps, once: from the tables for INTER_LINEAR, by arithmetic for the copy and the 2 x 2 mean
  if (t < xe - x0) {
    const int x = x0 + t;
    FnX e = {a.mode == RS_AREA2 ? 2 * x : x, 0};
    if (a.mode == RS_LINEAR) e = a.xt[x];
    sxt[t] = e;
  } else if (t >= 64 && t < 64 + FN_ROWS) {
    const int y = min(ty0 + t - 64, a.nh - 1);
    FnY e = {a.mode == RS_AREA2 ? 2 * y : y, a.mode == RS_AREA2 ? 2 * y + 1 : y, 0, 0};
    if (a.mode == RS_LINEAR) e = a.yt[y];
    syt[t - 64] = e;
  }
  __syncthreads();
  const int pmin = sxt[0].sx, pmax = min(sxt[xe - x0 - 1].sx + extra, a.sw - 1);
  const int b0 = a.vec_in ? (3 * pmin) & ~15 : 3 * pmin, b1 = 3 * pmax + 3;   // byte span of the source rows
  const size_t srow = (size_t)a.sw * 3;
  const int nrows = a.mode == RS_COPY ? FN_ROWS : 2 * FN_ROWS;
  if (a.vec_in) {
    const int nv = (b1 - b0 + 15) >> 4;   // <= 15 (the host chose cx so)
    for (int i = t; i < nrows * nv; i += 256) {
      const int r = i / nv, v = i - r * nv, lr = r & (FN_ROWS - 1);
      const FnY e = syt[lr];
      const int sy = r < FN_ROWS ? e.y0 : e.y1;
      // rows are multiples of 16 bytes here, so a vector that starts inside the row ends inside it
      const uint4 q = *reinterpret_cast<const uint4*>(src + (size_t)sy * srow + b0 + 16 * v);
      unsigned* d = rows + ((r & FN_ROWS) + (lr & 3) * 16 + (lr >> 2)) * FN_SEGD + 4 * v;
      d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    }
  } else {
    const int nb = b1 - b0;
    uint8_t* rb = reinterpret_cast<uint8_t*>(rows);
    for (int i = t; i < nrows * nb; i += 256) {
      const int r = i / nb, k = i - r * nb, lr = r & (FN_ROWS - 1);
      const FnY e = syt[lr];
      const int sy = r < FN_ROWS ? e.y0 : e.y1;
      rb[((r & FN_ROWS) + (lr & 3) * 16 + (lr >> 2)) * (FN_SEGD * 4) + k] = src[(size_t)sy * srow + b0 + k];
    }
  }
  __syncthreads();
  const int ly = t & 15, lx = t >> 4, y = ty0 + 4 * ly;
  if (y >= a.nh) return;   // nh is a multiple of 8: rows y .. y + 3 exist together
  float* __restrict__ dst = st_gl(a.dst[blockIdx.z]);
  const uint8_t* rb = reinterpret_cast<const uint8_t*>(rows);
  int wb0[4], wb1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const FnY e = syt[4 * ly + j];
    wb0[j] = e.b0; wb1[j] = e.b1;
  }
  for (int x = x0 + lx; x < xe; x += 16) {
    const FnX e = sxt[x - x0];
    const int o = 3 * e.sx - b0, a0 = e.a & 0xffff, a1 = e.a >> 16;
    const bool two = e.sx + 1 < a.sw;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint8_t* R0 = rb + (j * 16 + ly) * (FN_SEGD * 4) + o + c;
        const uint8_t* R1 = R0 + FN_ROWS * FN_SEGD * 4;
        int q;
        if (a.mode == RS_COPY) {
          q = R0[0];
        } else if (a.mode == RS_AREA2) {
          q = (R0[0] + R0[3] + R1[0] + R1[3] + 2) >> 2;
        } else {
          const int r0 = rs_linear_h(R0[0], two ? R0[3] : 0, a0, a1, two);
          const int r1 = rs_linear_h(R1[0], two ? R1[3] : 0, a0, a1, two);
          q = rs_linear_v(r0, r1, wb0[j], wb1[j]) & 0xff;
        }
        v[j] = (float)q - a.mean[c];
      }
      float* D = dst + ((size_t)c * a.nw + x) * a.nh + y;
      if (a.vec_out) {
        *reinterpret_cast<float4*>(D) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        D[0] = v[0]; D[1] = v[1]; D[2] = v[2]; D[3] = v[3];
      }
    }
  }
}

// ---- CaffeInput -----------------------------------------------------------------------------------
struct CfTap { int start, count; float weight; int pad; };   // first member's source index (before edge replication), members, 1 / members

struct CaffeK {
  const uint8_t* const* src;  // n RGB frames (sh, sw, 3)
  float* const* dst;          // n planar (3, nh, nw) float frames
  const CfTap* xt;            // nw entries
  const CfTap* yt;            // nh entries
  int sh, sw, nh, nw, cx, orows, seg, smax;
  int vec_in, normalize;
  float mean[3];
};

// A workgroup owns `orows` output rows x `cx` output columns and walks the source rows of its rows' windows once.  Each of
// its four waves takes every fourth source row on its own: it stages the row's byte span in its LDS slot (the next row's
// bytes are already on their way in registers), forms the row's horizontal sums rx (one float per channel and column) in
// LDS, and goes on -- no workgroup barrier until all rows are done; then the vertical sums over rx.  Every sum runs over
// the window's members in order, in float32, multiply and add rounded separately (the file is compiled with
// -ffp-contract=off).  Nothing is divided inside the loops.
// LDS: [cx CfTap][4 * seg staged bytes][smax * 3 * cx floats of rx]
constexpr int CF_WAVES = 4;
constexpr int CF_PRE = 7;    // 16-byte vectors a lane holds of its wave's next row: seg / 16 <= 448 (caffe_plan)

// LDS traffic of one wave is executed in order; this only keeps the compiler from moving it across
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(256) void k_caffe_input(CaffeK a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  CfTap* sxt = reinterpret_cast<CfTap*>(lds);
  uint8_t* stage = lds + (size_t)a.cx * sizeof(CfTap);
  float* rx = reinterpret_cast<float*>(stage + (size_t)CF_WAVES * a.seg);
  const int t = threadIdx.x, wv = t >> 6, ln = t & 63;
  const int x0 = blockIdx.x * a.cx, xe = min(x0 + a.cx, a.nw), ncx = xe - x0, ncols = 3 * ncx;
  const int r0 = blockIdx.y * a.orows, re = min(r0 + a.orows, a.nh);
  const uint8_t* __restrict__ src = st_gl(a.src[blockIdx.z]);
  for (int i = t; i < ncx; i += 256) sxt[i] = a.xt[x0 + i];
  const CfTap xl = a.xt[xe - 1], yf = a.yt[r0], yl = a.yt[re - 1];
  // The last member of a row's last window may be index sw (edge replication): the staged row then gets the edge pixel
  // once more behind its end, so that the sums below index without a clamp.  A window may even start there.
  const int last = xl.start + xl.count - 1;
  const int pmin = min(a.xt[x0].start, a.sw - 1), pmax = min(last, a.sw - 1);
  const int b0 = a.vec_in ? (3 * pmin) & ~15 : 3 * pmin, b1 = 3 * pmax + 3;
  const int ys = min(yf.start, a.sh - 1), ye = min(yl.start + yl.count - 1, a.sh - 1);   // source rows ys .. ye
  const size_t srow = (size_t)a.sw * 3;
  const int nv = (b1 - b0 + 15) >> 4, nb = b1 - b0;
  uint8_t* wstage = stage + (size_t)wv * a.seg;
  __syncthreads();   // sxt
  uint4 pre[CF_PRE];
  auto fetch = [&](int row) {
#pragma unroll
    for (int u = 0; u < CF_PRE; ++u)
      if (ln + 64 * u < nv) pre[u] = *reinterpret_cast<const uint4*>(src + (size_t)row * srow + b0 + 16 * (ln + 64 * u));
  };
  if (a.vec_in && ys + wv <= ye) fetch(ys + wv);
  for (int row = ys + wv; row <= ye; row += CF_WAVES) {
    wave_lds_fence();   // the previous row's bytes have been read
    if (a.vec_in) {
#pragma unroll
      for (int u = 0; u < CF_PRE; ++u)
        if (ln + 64 * u < nv) *reinterpret_cast<uint4*>(wstage + 16 * (ln + 64 * u)) = pre[u];
    } else {
      for (int k = ln; k < nb; k += 64) wstage[k] = src[(size_t)row * srow + b0 + k];
    }
    // the replicated edge pixel at index sw (no staged vector reaches it)
    if (last >= a.sw && ln < 3) wstage[3 * a.sw + ln - b0] = src[(size_t)row * srow + 3 * (a.sw - 1) + ln];
    wave_lds_fence();
    if (a.vec_in && row + CF_WAVES <= ye) fetch(row + CF_WAVES);
    float* rxr = rx + (size_t)(row - ys) * ncols;
    for (int x = ln; x < ncx; x += 64) {
      const CfTap e = sxt[x];
      const uint8_t* S = wstage + 3 * e.start - b0;
      float acc[3] = {0.f, 0.f, 0.f};
      // four members at a time: their twelve bytes are read before any is added (a read past the window's end repeats its
      // last member and is not added), so the LDS latency is paid once per four; the order of the additions is unchanged
      for (int k0 = 0; k0 < e.count; k0 += 4) {
        float v[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint8_t* P = S + 3 * min(k0 + j, e.count - 1);
#pragma unroll
          for (int c = 0; c < 3; ++c) v[j][c] = (float)P[c];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k0 + j < e.count) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + e.weight * v[j][c];
          }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) rxr[c * ncx + x] = acc[c];
    }
  }
  __syncthreads();
  float* __restrict__ dst = st_gl(a.dst[blockIdx.z]);
  for (int r = r0; r < re; ++r) {
    const CfTap e = a.yt[r];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int co = 2 - c;   // output plane co holds input channel 2 - co
      for (int x = t; x < ncx; x += 256) {
        const float* R = rx + c * ncx + x;
        float acc = 0.f;
        for (int k0 = 0; k0 < e.count; k0 += 4) {   // as above: four reads, then up to four additions in order
          float v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = R[(size_t)(min(e.start + min(k0 + j, e.count - 1), a.sh - 1) - ys) * ncols];
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (k0 + j < e.count) acc = acc + e.weight * v[j];
        }
        acc = fminf(fmaxf(acc, 0.0f), 255.0f);
        float v = acc - a.mean[co];
        if (a.normalize) v = v / 255.0f;
        dst[((size_t)co * a.nh + r) * a.nw + x0 + x] = v;
      }
    }
  }
}

// the device buffer of a plan holds `bytes`
int plan_reserve(st_ctx* ctx, st_netin_plan* p, size_t bytes) {
  if (bytes <= p->dev_bytes) return ST_OK;
  ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (p->dev) ST_HIP(ctx, hipFree(p->dev));
  p->dev = nullptr;
  p->dev_bytes = 0;
  p->h = 0;
  const hipError_t e = hipMalloc(&p->dev, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    p->dev = nullptr;
    return st_set_error(ctx, ST_ERR_OOM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  }
  p->dev_bytes = bytes;
  return ST_OK;
}

bool all_aligned16(const void* const* p, int n) {
  for (int i = 0; i < n; ++i)
    if ((uintptr_t)p[i] & 15) return false;
  return true;
}

// the tables and the tile width of FacenetInput for one geometry, uploaded on the context's stream
int facenet_plan(st_ctx* ctx, int h, int w, int nh, int nw) {
  if (!ctx->netin) ctx->netin = new st_netin_state();
  st_netin_plan& p = ctx->netin->facenet;
  if (p.h == h && p.w == w && p.nh == nh && p.nw == nw) return ST_OK;
  const st_rs_scales s = st_rs_plan_scales(h, w, nh, nw);
  const int mode = st_rs_linear_mode(h, w, nh, nw, s);
  std::vector<FnX> xt(nw);
  std::vector<FnY> yt(nh);
  for (int x = 0; x < nw; ++x) {
    if (mode == RS_COPY) xt[x] = {x, 0};
    else if (mode == RS_AREA2) xt[x] = {2 * x, 0};
    else {
      int sx;
      const float fx = rs_linear_coord(x, s.scale_x, &sx);
      const RsTapX tx = rs_linear_tap_x(sx, fx, w);
      xt[x] = {tx.sx, tx.a0 | (tx.a1 << 16)};
    }
  }
  for (int y = 0; y < nh; ++y) {
    if (mode == RS_COPY) yt[y] = {y, y, 0, 0};
    else if (mode == RS_AREA2) yt[y] = {2 * y, 2 * y + 1, 0, 0};
    else {
      int sy;
      const float fy = rs_linear_coord(y, s.scale_y, &sy);
      const RsTapY ty = rs_linear_tap_y(sy, fy, h);
      yt[y] = {ty.y0, ty.y1, ty.b0, ty.b1};
    }
  }
  // the widest tile whose source byte span (from a 16-byte boundary) fits a staged row; one column always fits
  const int extra = mode == RS_COPY ? 0 : 1;
  int cx = FN_MAX_CX;
  for (; cx > 1; --cx) {
    bool fits = true;
    for (int x0 = 0; x0 < nw && fits; x0 += cx) {
      const int xe = x0 + cx < nw ? x0 + cx : nw;
      const int pmax = xt[xe - 1].sx + extra < w - 1 ? xt[xe - 1].sx + extra : w - 1;
      fits = 3 * pmax + 3 - ((3 * xt[x0].sx) & ~15) <= FN_SEG_BYTES;
    }
    if (fits) break;
  }
  const size_t y_off = st_align_up(sizeof(FnX) * (size_t)nw);
  ST_TRY(plan_reserve(ctx, &p, y_off + sizeof(FnY) * (size_t)nh));
  p.h = 0;
  ST_HIP(ctx, hipMemcpyAsync(p.dev, xt.data(), sizeof(FnX) * xt.size(), hipMemcpyHostToDevice, ctx->stream));
  ST_HIP(ctx, hipMemcpyAsync((char*)p.dev + y_off, yt.data(), sizeof(FnY) * yt.size(), hipMemcpyHostToDevice, ctx->stream));
  p.y_off = y_off; p.mode = mode; p.cx = cx;
  p.h = h; p.w = w; p.nh = nh; p.nw = nw;
  return ST_OK;
}

constexpr int CF_SEG_MAX = 6144;          // bytes of a source row a wave stages (a 1920-pixel row is 5760); seg <= 6176 = 386 vectors <= 64 CF_PRE
constexpr size_t CF_LDS_MAX = 64 * 1024;  // LDS of one workgroup

int axis_taps(int n_in, int n_out, std::vector<CfTap>* t) {
  std::vector<int> begin(n_out), first(n_out), count(n_out);
  const int st = st_caffe_input_axis(n_in, n_out, begin.data(), first.data(), count.data());
  if (st != ST_OK) return st;
  t->resize(n_out);
  for (int i = 0; i < n_out; ++i) {
    (*t)[i] = {begin[i] + first[i], count[i], 1.0f / (float)count[i], 0};
    // the kernel takes a tile's source span from its first and last window: both ends must move forward only
    if (i && ((*t)[i].start < (*t)[i - 1].start || (*t)[i].start + count[i] < (*t)[i - 1].start + count[i - 1])) return ST_ERR_UNSUPPORTED;
    if ((*t)[i].start + count[i] - 1 > n_in) return ST_ERR_UNSUPPORTED;   // index n_in is the replicated edge; nothing lies beyond
  }
  return ST_OK;
}

// the tables and the tiling of CaffeInput for one geometry; the status of a refused geometry is cached too
int caffe_plan(st_ctx* ctx, int h, int w, int nh, int nw) {
  if (!ctx->netin) ctx->netin = new st_netin_state();
  st_netin_plan& p = ctx->netin->caffe;
  if (p.h == h && p.w == w && p.nh == nh && p.nw == nw) return p.status;
  std::vector<CfTap> xt, yt;
  int st = axis_taps(w, nw, &xt);
  if (st == ST_OK) st = axis_taps(h, nh, &yt);
  if (st != ST_OK) {
    p.h = h; p.w = w; p.nh = nh; p.nw = nw; p.status = st;
    return st;
  }
  // widest source byte span of a chunk of cx columns, from a 16-byte boundary; most source rows under `orows` output rows
  auto span = [&](int cx) {
    int m = 0;
    for (int x0 = 0; x0 < nw; x0 += cx) {
      const CfTap& l = xt[(x0 + cx < nw ? x0 + cx : nw) - 1];
      const int pmax = l.start + l.count - 1 < w - 1 ? l.start + l.count - 1 : w - 1;
      m = std::max(m, 3 * pmax + 3 - ((3 * std::min(xt[x0].start, w - 1)) & ~15));
    }
    return m;
  };
  auto rows_under = [&](int orows) {
    int m = 0;
    for (int r0 = 0; r0 < nh; r0 += orows) {
      const CfTap& l = yt[(r0 + orows < nh ? r0 + orows : nh) - 1];
      const int ye = l.start + l.count - 1 < h - 1 ? l.start + l.count - 1 : h - 1;
      m = std::max(m, ye - std::min(yt[r0].start, h - 1) + 1);
    }
    return m;
  };
  int cx = nw < 256 ? nw : 256;
  while (cx > 1 && span(cx) > CF_SEG_MAX) cx = (cx + 1) / 2;
  int orows = 0, seg = 0, smax = 0;
  size_t lds = 0;
  for (;;) {
    if (span(cx) > CF_SEG_MAX) break;   // one column's window is wider than a staged row
    seg = (span(cx) + 3 + 15) / 16 * 16;   // + the replicated edge pixel behind the row's end
    for (orows = 4; orows >= 1; orows /= 2) {
      smax = rows_under(orows);
      lds = sizeof(CfTap) * (size_t)cx + (size_t)CF_WAVES * seg + sizeof(float) * 3 * (size_t)cx * smax;
      if (lds <= CF_LDS_MAX) break;
    }
    if (orows >= 1 || cx == 1) break;
    cx = (cx + 1) / 2;
  }
  if (orows < 1 || span(cx) > CF_SEG_MAX) {
    p.h = 0;
    return st_set_error(ctx, ST_ERR_UNSUPPORTED, "caffe_input: %dx%d -> %dx%d needs windows larger than a workgroup's LDS", w, h, nw, nh);
  }
  const size_t y_off = st_align_up(sizeof(CfTap) * (size_t)nw);
  ST_TRY(plan_reserve(ctx, &p, y_off + sizeof(CfTap) * (size_t)nh));
  p.h = 0;
  ST_HIP(ctx, hipMemcpyAsync(p.dev, xt.data(), sizeof(CfTap) * xt.size(), hipMemcpyHostToDevice, ctx->stream));
  ST_HIP(ctx, hipMemcpyAsync((char*)p.dev + y_off, yt.data(), sizeof(CfTap) * yt.size(), hipMemcpyHostToDevice, ctx->stream));
  p.y_off = y_off; p.cx = cx; p.orows = orows; p.seg = seg; p.smax = smax; p.lds = lds;
  p.status = ST_OK;
  p.h = h; p.w = w; p.nh = nh; p.nw = nw;
  return ST_OK;
}

}  // namespace

ST_EXPORT int st_facenet_geometry(int h, int w, float scale, int* net_h, int* net_w) {
  if (h <= 0 || w <= 0 || !(scale > 0)) return ST_ERR_INVALID;
  // facenet_input_kernel_cpu.cpp:22-29: std::floor(i32 * f32) (a float product), then padding to a multiple of 8
  const float fw = floorf((float)w * scale), fh = floorf((float)h * scale);
  if (!(fw >= 1.f) || !(fh >= 1.f) || fw > 1e8f || fh > 1e8f) return ST_ERR_INVALID;
  int nw = (int)fw, nh = (int)fh;
  if (nw % 8) nw += 8 - nw % 8;
  if (nh % 8) nh += 8 - nh % 8;
  if (net_h) *net_h = nh;
  if (net_w) *net_w = nw;
  return ST_OK;
}

ST_EXPORT int st_facenet_input_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, float scale,
                                     const float* mean, float* const* out_dev) {
  ST_TRY(st_enter(ctx));
  int nh, nw;
  if (n < 0 || !mean || st_facenet_geometry(h, w, scale, &nh, &nw) != ST_OK || (long long)h * w > 200000000LL ||
      (long long)nh * nw > 200000000LL)
    return st_set_error(ctx, ST_ERR_INVALID, "facenet_input: bad arguments (n=%d h=%d w=%d scale=%g)", n, h, w, (double)scale);
  if ((nh + FN_ROWS - 1) / FN_ROWS > 65535) return st_set_error(ctx, ST_ERR_UNSUPPORTED, "facenet_input: network input too tall");
  if (n == 0) return ST_OK;
  if (!frames_dev || !out_dev) return st_set_error(ctx, ST_ERR_INVALID, "facenet_input: null argument");
  ST_TRY(st_check_rows(ctx, "facenet_input: row %d is null", n, false, frames_dev, out_dev));
  ST_TRY(facenet_plan(ctx, h, w, nh, nw));
  const st_netin_plan& p = ctx->netin->facenet;
  const uint8_t** d_src;
  float** d_dst;
  ST_TRY(st_upload_tables(ctx, n, 0, frames_dev, &d_src, out_dev, &d_dst));
  FacenetK a;
  a.xt = (const FnX*)p.dev; a.yt = (const FnY*)((const char*)p.dev + p.y_off);
  a.sh = h; a.sw = w; a.nh = nh; a.nw = nw; a.cx = p.cx; a.mode = p.mode;
  a.vec_in = (3 * (long long)w) % 16 == 0 && all_aligned16((const void* const*)frames_dev, n);
  a.vec_out = all_aligned16((const void* const*)out_dev, n);
  a.mean[0] = mean[0]; a.mean[1] = mean[1]; a.mean[2] = mean[2];
  return st_for_launches(n, [&](int f0, int nf) -> int {
    a.src = d_src + f0; a.dst = d_dst + f0;
    st_timed t(ctx, ST_K_NET_INPUT);
    hipLaunchKernelGGL(k_facenet_input, dim3((nw + p.cx - 1) / p.cx, (nh + FN_ROWS - 1) / FN_ROWS, nf), dim3(256), 0, ctx->stream, a);
    ST_HIP(ctx, hipGetLastError());
    return ST_OK;
  });
}

ST_EXPORT int st_caffe_input_axis(int n_in, int n_out, int* begin, int* first, int* count) {
  if (n_in <= 0 || n_out <= 0 || n_in > (1 << 24) || n_out > (1 << 24) || !begin || !first || !count) return ST_ERR_INVALID;
  // caffe_input_transformer_base.h:51-70, one axis: every operation an IEEE float32 operation
  const float scale = (float)n_out / (float)n_in;
  const float ks = 0.5f / scale;
  const int extent = (int)(2.0f * ks + 1.0f);
  int status = ST_OK;
  for (int x = 0; x < n_out; ++x) {
    const float src = ((float)x + 0.5f) / scale;
    const int b = (int)(src - ks + 0.5f);
    int f = -1, m = 0, last = -1;
    for (int k = 0; k < extent; ++k)
      if (fabsf(((float)(k + b) - src) * scale) <= 0.5f) {
        if (f < 0) f = k;
        last = k;
        ++m;
      }
    begin[x] = b; first[x] = f; count[x] = m;
    // an empty window (the reference divides 0 by 0), members that are not contiguous, or a window left of the row
    if (m == 0 || last - f + 1 != m || b + f < 0) status = ST_ERR_UNSUPPORTED;
  }
  return status;
}

ST_EXPORT int st_caffe_input_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int net_h, int net_w,
                                   const float* mean_bgr, int normalize, float* const* out_dev) {
  ST_TRY(st_enter(ctx));
  if (n < 0 || h <= 0 || w <= 0 || net_h <= 0 || net_w <= 0 || !mean_bgr || (long long)h * w > 200000000LL ||
      (long long)net_h * net_w > 200000000LL)
    return st_set_error(ctx, ST_ERR_INVALID, "caffe_input: bad arguments (n=%d %dx%d -> %dx%d)", n, h, w, net_h, net_w);
  if (net_h > 65535) return st_set_error(ctx, ST_ERR_UNSUPPORTED, "caffe_input: network input taller than 65535 rows");
  // the geometry is judged before anything else happens, an empty batch included
  const int st = caffe_plan(ctx, h, w, net_h, net_w);
  if (st == ST_ERR_UNSUPPORTED && ctx->netin->caffe.h == h)
    return st_set_error(ctx, ST_ERR_UNSUPPORTED, "caffe_input: %dx%d -> %dx%d has an empty or irregular filter window (the reference divides 0 by 0 in an empty one); "
                        "only downscales, equal sizes and integer enlargements are supported", w, h, net_w, net_h);
  if (st != ST_OK) return st;
  if (n == 0) return ST_OK;
  if (!frames_dev || !out_dev) return st_set_error(ctx, ST_ERR_INVALID, "caffe_input: null argument");
  ST_TRY(st_check_rows(ctx, "caffe_input: row %d is null", n, false, frames_dev, out_dev));
  const st_netin_plan& p = ctx->netin->caffe;
  const uint8_t** d_src;
  float** d_dst;
  ST_TRY(st_upload_tables(ctx, n, 0, frames_dev, &d_src, out_dev, &d_dst));
  CaffeK a;
  a.xt = (const CfTap*)p.dev; a.yt = (const CfTap*)((const char*)p.dev + p.y_off);
  a.sh = h; a.sw = w; a.nh = net_h; a.nw = net_w; a.cx = p.cx; a.orows = p.orows; a.seg = p.seg; a.smax = p.smax;
  a.vec_in = (3 * (long long)w) % 16 == 0 && all_aligned16((const void* const*)frames_dev, n);
  a.normalize = normalize != 0;
  a.mean[0] = mean_bgr[0]; a.mean[1] = mean_bgr[1]; a.mean[2] = mean_bgr[2];
  return st_for_launches(n, [&](int f0, int nf) -> int {
    a.src = d_src + f0; a.dst = d_dst + f0;
    st_timed t(ctx, ST_K_NET_INPUT);
    hipLaunchKernelGGL(k_caffe_input, dim3((net_w + p.cx - 1) / p.cx, (net_h + p.orows - 1) / p.orows, nf), dim3(256), p.lds, ctx->stream, a);
    ST_HIP(ctx, hipGetLastError());
    return ST_OK;
  });
}
