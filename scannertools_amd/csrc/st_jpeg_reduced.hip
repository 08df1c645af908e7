// ImageDecoder at scale 1/2, 1/4 and 1/8: the dense stages of st_jpeg.hip with libjpeg's reduced inverse DCTs (jidctint's
// 4 x 4 and 2 x 2, the 1 x 1 DC-only one) in place of the 8 x 8 one.  Entropy decoding and the upload are unchanged, so the
// kernels here read the same headers and coefficients and launch in the same place (DESIGN.md 4.12c has the contract).
//   k_jpeg_idct_reduced  blocks whose component decodes at S = 2, 4 or 8 samples a side: one lane per block row, as k_jpeg_idct
//   k_jpeg_idct_1x1      blocks whose component decodes at S = 1: one lane per block, no LDS
//   k_jpeg_color_reduced the h2v1 upsampling that is left at 4:2:2 + YCbCr -> RGB into the dense reduced frames
// Plane layout: a frame keeps its place in the planes buffer (blk_off * 64, so the buffer's size and the frames' offsets are the
// full-size path's) and its component planes are block-tiled DENSELY inside it, S * S bytes per block: sample (y, x) of a
// component is byte (y % S) * S + (x % S) of block (y / S) * blocks_per_row + (x / S), and a component's plane starts on the next
// multiple of 64 bytes behind the one before it (red_plane_bytes).  At S = 1 a plane is a plain raster of its blocks.
#include "st_internal.h"
#include "st_jpeg_dense.h"
#include "st_jpeg_parse.h"

namespace {

// bytes of a component plane of nblk blocks of S x S samples, rounded up so that the next plane stays 64-byte aligned; never
// more than the 64 bytes per block the buffer has
__device__ __forceinline__ size_t red_plane_bytes(int nblk, int S) { return ((size_t)nblk * (size_t)(S * S) + 63) & ~(size_t)63; }

// where block b (of the frame's ny luma and 2 nc chroma blocks) of S x S samples starts, relative to the frame's first byte
__device__ __forceinline__ size_t red_block_at(int b, int ny, int nc, int sy, int sc) {
  if (b < ny) return (size_t)b * (size_t)(sy * sy);
  const size_t pc = red_plane_bytes(nc, sc);
  return red_plane_bytes(ny, sy) + (b >= ny + nc ? pc : 0) + (size_t)(b - ny - (b >= ny + nc ? nc : 0)) * (size_t)(sc * sc);
}

// jpeg_idct_4x4's pass over 8 inputs (entry 4 is not read): 4 outputs, DESCALE by n
__device__ __forceinline__ void idct_pass4(const int* i, int* o, int n) {
  const int t0 = i[0] * 16384;
  const int t2 = 15137 * i[2] - 6270 * i[6];
  const int t10 = t0 + t2, t12 = t0 - t2;
  const int a = -1730 * i[7] + 11893 * i[5] - 17799 * i[3] + 8697 * i[1];
  const int b = -4176 * i[7] - 4926 * i[5] + 7373 * i[3] + 20995 * i[1];
  const int r = 1 << (n - 1);
  o[0] = (t10 + b + r) >> n; o[3] = (t10 - b + r) >> n;
  o[1] = (t12 + a + r) >> n; o[2] = (t12 - a + r) >> n;
}

// jpeg_idct_2x2's pass (entries 0, 1, 3, 5 and 7 are read): 2 outputs
__device__ __forceinline__ void idct_pass2(const int* i, int* o, int n) {
  const int t10 = i[0] * 32768;
  const int t0 = -5906 * i[7] + 6967 * i[5] - 10426 * i[3] + 29692 * i[1];
  const int r = 1 << (n - 1);
  o[0] = (t10 + t0 + r) >> n;
  o[1] = (t10 - t0 + r) >> n;
}

// Lane = (block, r) as in k_jpeg_idct: it loads coefficient row r where the transform of size S reads that row, runs pass 1
// on column r where pass 2 reads that column, and pass 2 on row r of the pass-1 result where r < S; the other lanes of a
// block sit idle.  The rows and columns read: all 8 at S = 8, all but 4 at S = 4, {0, 1, 3, 5, 7} at S = 2.  Blocks of a
// component that decodes at S = 1 are k_jpeg_idct_1x1's: a frame whose luma does starts behind its luma plane here.
constexpr int kIdctBlocks = 32, kLdsBlock = 72;
__global__ __launch_bounds__(256) void k_jpeg_idct_reduced(JpegArgsK a) {
  __shared__ int lds[kIdctBlocks * kLdsBlock];
  const JpegFrameHdr* __restrict__ hdr = reinterpret_cast<const JpegFrameHdr*>(a.slot) + blockIdx.y;
  const int ny = hdr->nblk_y, nc = hdr->nblk_c;
  const int total = ny + 2 * nc;
  const int lb = threadIdx.x >> 3, r = threadIdx.x & 7;
  const int b = (hdr->s_y == 1 ? ny : 0) + blockIdx.x * kIdctBlocks + lb;
  const int comp = (b >= ny) + (b >= ny + nc);
  int S = b < total ? (comp ? hdr->s_c : hdr->s_y) : 0;
  if (S < 2) S = 0;
  const unsigned reads = S == 8 ? 0xffu : (S == 4 ? 0xefu : (S == 2 ? 0xabu : 0u));
  const bool mine = (reads >> r) & 1;
  const size_t blk = (size_t)hdr->blk_off + (size_t)(S ? b : 0);
  int v[8], t[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { v[k] = 0; t[k] = 0; }
  if (mine) {
    const short8 c = *reinterpret_cast<const short8*>(a.slot + (size_t)a.nf * sizeof(JpegFrameHdr) + blk * 128 + (size_t)r * 16);
    const ushort8 q = *reinterpret_cast<const ushort8*>(&hdr->quant[comp][r * 8]);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (int)c[k] * (int)q[k];
  }
  int* L = lds + lb * kLdsBlock;
#pragma unroll
  for (int k = 0; k < 8; ++k) L[r * 8 + k] = v[k];
  __syncthreads();
  if (mine) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = L[k * 8 + r];   // column r
    if (S == 8) idct_pass(v, t, 11);
    else if (S == 4) idct_pass4(v, t, 12);
    else idct_pass2(v, t, 13);
  }
  __syncthreads();
  if (mine) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < S) L[k * 8 + r] = t[k];
  }
  __syncthreads();
  if (r < S) {
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = L[r * 8 + k];   // row r of the pass-1 result
    uint8_t* dst = a.planes + (size_t)hdr->blk_off * 64 + red_block_at(b, ny, nc, hdr->s_y, hdr->s_c) + (size_t)(r * S);
    if (S == 8) {
      idct_pass(v, t, 18);
      unsigned lo = 0, hi = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        lo |= (unsigned)clamp255(t[k] + 128) << (8 * k);
        hi |= (unsigned)clamp255(t[4 + k] + 128) << (8 * k);
      }
      *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
    } else if (S == 4) {
      idct_pass4(v, t, 19);
      unsigned lo = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) lo |= (unsigned)clamp255(t[k] + 128) << (8 * k);
      *reinterpret_cast<unsigned*>(dst) = lo;
    } else {
      idct_pass2(v, t, 20);
      *reinterpret_cast<unsigned short*>(dst) = (unsigned short)(clamp255(t[0] + 128) | (clamp255(t[1] + 128) << 8));
    }
  }
}

// One lane per block of a component that decodes at S = 1: DESCALE(coef[0] * quant[0], 3), one byte out.
__global__ __launch_bounds__(256) void k_jpeg_idct_1x1(JpegArgsK a) {
  const JpegFrameHdr* __restrict__ hdr = reinterpret_cast<const JpegFrameHdr*>(a.slot) + blockIdx.y;
  const int ny = hdr->nblk_y, nc = hdr->nblk_c;
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= ny + 2 * nc) return;
  const int comp = (b >= ny) + (b >= ny + nc);
  if ((comp ? hdr->s_c : hdr->s_y) != 1) return;
  const size_t blk = (size_t)hdr->blk_off + (size_t)b;
  const int c = *reinterpret_cast<const short*>(a.slot + (size_t)a.nf * sizeof(JpegFrameHdr) + blk * 128);
  a.planes[(size_t)hdr->blk_off * 64 + red_block_at(b, ny, nc, hdr->s_y, hdr->s_c)] = (uint8_t)clamp255(((c * (int)hdr->quant[comp][0] + 4) >> 3) + 128);
}

// ---- upsampling + colour ----------------------------------------------------------------------------------------------------
// a plane of blocks of S = 1 << ls samples a side
struct RedPlane { const uint8_t* __restrict__ p; int bw, ls; };

__device__ __forceinline__ size_t smp_at(const RedPlane& P, int y, int x) {
  const int m = (1 << P.ls) - 1;
  return (((size_t)(y >> P.ls) * P.bw + (size_t)(x >> P.ls)) << (2 * P.ls)) + (size_t)(((y & m) << P.ls) + (x & m));
}

struct RedChroma { int ups, fancy, dw; };

// One chroma sample at the reduced frame's resolution: the plane's own, or h2v1 from it -- (3 p[i] + p[i -/+ 1] + 1 / 2) >> 2,
// the neighbour clamped into the plane (libjpeg's edge columns) or replaced by the sample itself (its plain replication).
__device__ __forceinline__ int chroma_at(const RedPlane& P, const RedChroma& g, int y, int x) {
  if (g.ups == 1) return P.p[smp_at(P, y, x)];
  const int i = x >> 1;
  int j = i + ((x & 1) ? 1 : -1);
  j = j < 0 ? 0 : (j > g.dw - 1 ? g.dw - 1 : j);
  if (!g.fancy) j = i;
  return (3 * P.p[smp_at(P, y, i)] + P.p[smp_at(P, y, j)] + ((x & 1) ? 2 : 1)) >> 2;
}

// four samples of one row from x (a multiple of 4): one dword where a block row holds them, two 16-bit loads at S = 2, bytes at S = 1
__device__ __forceinline__ void load4(const RedPlane& P, int y, int x, int* o) {
  if (P.ls >= 2) {
    const unsigned v = *reinterpret_cast<const unsigned*>(P.p + smp_at(P, y, x));
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (v >> (8 * k)) & 0xff;
  } else if (P.ls == 1) {
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
      const unsigned v = *reinterpret_cast<const unsigned short*>(P.p + smp_at(P, y, x + k));
      o[k] = v & 0xff;
      o[k + 1] = v >> 8;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = P.p[smp_at(P, y, x + k)];
  }
}

// PX pixels of one row of the reduced frame per thread, chosen as k_jpeg_color's on the reduced width: PX = 16: w % 16 == 0 and
// 16-byte aligned frames; PX = 4: w % 4 == 0 and 4-byte aligned frames; PX = 1: anything.
template <int PX>
__global__ __launch_bounds__(256) void k_jpeg_color_reduced(JpegArgsK a) {
  const JpegFrameHdr* __restrict__ hdr = reinterpret_cast<const JpegFrameHdr*>(a.slot) + blockIdx.y;
  const int lsy = hdr->s_y == 8 ? 3 : (hdr->s_y == 4 ? 2 : (hdr->s_y == 2 ? 1 : 0));
  const int lsc = hdr->s_c == 8 ? 3 : (hdr->s_c == 4 ? 2 : (hdr->s_c == 2 ? 1 : 0));
  const RedPlane PY{a.planes + (size_t)hdr->blk_off * 64, hdr->bw_y, lsy};
  const RedPlane PB{PY.p + red_plane_bytes(hdr->nblk_y, hdr->s_y), hdr->bw_c, lsc};
  const RedPlane PR{PB.p + red_plane_bytes(hdr->nblk_c, hdr->s_c), hdr->bw_c, lsc};
  RedChroma g;
  g.ups = hdr->ups; g.fancy = hdr->fancy; g.dw = hdr->dw;
  uint8_t* __restrict__ out = st_gl(hdr->out);
  const int w = a.w, cn = a.channels;
  const long long groups = (long long)a.h * w / PX;
  for (long long gi = (long long)blockIdx.x * 256 + threadIdx.x; gi < groups; gi += (long long)gridDim.x * 256) {
    const long long pix = gi * PX;
    const int y = (int)(pix / w), x0 = (int)(pix % w);
    int Y[PX], Cb[PX], Cr[PX];
    if constexpr (PX == 1) {
      Y[0] = PY.p[smp_at(PY, y, x0)];
      if (cn == 3) {
        Cb[0] = chroma_at(PB, g, y, x0);
        Cr[0] = chroma_at(PR, g, y, x0);
      }
    } else {
#pragma unroll
      for (int q = 0; q < PX; q += 4) {
        load4(PY, y, x0 + q, Y + q);
        if (cn == 3) {
          if (g.ups == 1) {
            load4(PB, y, x0 + q, Cb + q);
            load4(PR, y, x0 + q, Cr + q);
          } else {
#pragma unroll
            for (int p = q; p < q + 4; ++p) {
              Cb[p] = chroma_at(PB, g, y, x0 + p);
              Cr[p] = chroma_at(PR, g, y, x0 + p);
            }
          }
        }
      }
    }
    if constexpr (PX == 1) {
      if (cn == 1) {
        out[pix] = (uint8_t)Y[0];
      } else {
        int rgb[3];
        ycc_rgb(Y[0], Cb[0], Cr[0], rgb);
        out[3 * pix] = (uint8_t)rgb[0]; out[3 * pix + 1] = (uint8_t)rgb[1]; out[3 * pix + 2] = (uint8_t)rgb[2];
      }
    } else if (cn == 1) {
      unsigned o[PX / 4];
#pragma unroll
      for (int k = 0; k < PX / 4; ++k) o[k] = 0;
#pragma unroll
      for (int p = 0; p < PX; ++p) o[p >> 2] |= (unsigned)Y[p] << (8 * (p & 3));
      if constexpr (PX == 16) *reinterpret_cast<uint4*>(out + pix) = make_uint4(o[0], o[1], o[2], o[3]);
      else *reinterpret_cast<unsigned*>(out + pix) = o[0];
    } else {
      constexpr int NO = 3 * PX / 4;
      unsigned o[NO];
#pragma unroll
      for (int k = 0; k < NO; ++k) o[k] = 0;
#pragma unroll
      for (int p = 0; p < PX; ++p) {
        int rgb[3];
        ycc_rgb(Y[p], Cb[p], Cr[p], rgb);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[(3 * p + k) >> 2] |= (unsigned)rgb[k] << (8 * ((3 * p + k) & 3));
      }
      unsigned* d = reinterpret_cast<unsigned*>(out + 3 * pix);
      if constexpr (PX == 16) {
#pragma unroll
        for (int k = 0; k < NO / 4; ++k) reinterpret_cast<uint4*>(d)[k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
      } else {
#pragma unroll
        for (int k = 0; k < NO; ++k) d[k] = o[k];
      }
    }
  }
}

}  // namespace

void st_jpeg_reduced_launch(st_ctx* ctx, const JpegArgsK& a, int nfl, size_t most1, size_t mostlds, int px) {
  if (most1) hipLaunchKernelGGL(k_jpeg_idct_1x1, dim3((unsigned)((most1 + 255) / 256), nfl), dim3(256), 0, ctx->stream, a);
  if (mostlds) hipLaunchKernelGGL(k_jpeg_idct_reduced, dim3((unsigned)((mostlds + kIdctBlocks - 1) / kIdctBlocks), nfl), dim3(256), 0, ctx->stream, a);
  long long bx = ((long long)a.h * a.w / px + 255) / 256;
  if (bx > 8192) bx = 8192;
  const dim3 grid((unsigned)bx, nfl);
  if (px == 16) hipLaunchKernelGGL(k_jpeg_color_reduced<16>, grid, dim3(256), 0, ctx->stream, a);
  else if (px == 4) hipLaunchKernelGGL(k_jpeg_color_reduced<4>, grid, dim3(256), 0, ctx->stream, a);
  else hipLaunchKernelGGL(k_jpeg_color_reduced<1>, grid, dim3(256), 0, ctx->stream, a);
}
