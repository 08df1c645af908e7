// ImageDecoder op, baseline JPEG: st_jpeg_decode_batch and its two kernels, and st_jpeg_decode_batch_gpu, the same call with the
// entropy decoding on the device too (k_jpeg_entropy_dec, st_jpeg_entropy.hip) for streams with restart intervals; its part
// of this file is at the end.
//
// Stage 1 (st_jpeg_parse.cpp, host threads) turns each stream into int16 coefficient blocks; this file uploads them and runs
//   k_jpeg_idct   dequantisation + libjpeg's "islow" inverse DCT, one lane per block row, into block-tiled component planes
//   k_jpeg_color  chroma upsampling ("fancy" triangle filter, or replication for planes at most 2 samples wide) + YCbCr -> RGB
//                 into the dense output frames
// Two launches per sub-batch (the unfused form; DESIGN.md 4.12 has the byte model).  The arithmetic is libjpeg's at its
// defaults (JDCT_ISLOW, fancy upsampling), restated in include/scannertools_hip.h's terms and DESIGN.md 4.12; the one known
// deviation is that samples are clamped where libjpeg's range table wraps (corrupt input only).
//
// Device layout of a sub-batch of nf frames (the page-locked slot holds the same bytes, one copy moves them):
//   [nf x JpegFrameHdr (512 B)] [coefficients: frame 0's blocks, frame 1's, ...]   128 B per block, natural order
// and the planes buffer holds 64 B per block in the SAME block order (component planes are block-tiled: sample (y, x) of a
// component is byte (y & 7) * 8 + (x & 7) of block (y >> 3) * blocks_per_row + (x >> 3)), so the IDCT kernel needs no plane
// geometry and a wave's eight blocks are 1 KiB of contiguous loads and 512 B of contiguous stores.
#include <algorithm>
#include <atomic>
#include <climits>
#include <cstring>
#include <mutex>
#include <thread>

#include "st_host_pipeline.h"
#include "st_internal.h"
#include "st_jpeg_dense.h"
#include "st_jpeg_entropy.h"
#include "st_jpeg_parse.h"

namespace {

// Lane = one row of one block: 16 B of coefficients in, 8 B of samples out; 32 blocks per workgroup, 8 per wave.  The two
// transposes (rows -> columns for pass 1, back for pass 2) go through LDS, 72 dwords per block: lanes (block, c) of a
// 32-lane half then touch 32 distinct banks on the strided side.
constexpr int kIdctBlocks = 32, kLdsBlock = 72;
__global__ __launch_bounds__(256) void k_jpeg_idct(JpegArgsK a) {
  __shared__ int lds[kIdctBlocks * kLdsBlock];
  const JpegFrameHdr* __restrict__ hdr = reinterpret_cast<const JpegFrameHdr*>(a.slot) + blockIdx.y;
  const int ny = hdr->nblk_y, nc = hdr->nblk_c;
  const int total = ny + 2 * nc;
  const int lb = threadIdx.x >> 3, r = threadIdx.x & 7;
  const int b = blockIdx.x * kIdctBlocks + lb;
  const bool live = b < total;
  const size_t blk = (size_t)hdr->blk_off + (size_t)(live ? b : 0);
  int v[8], t[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = 0;
  if (live) {
    const int comp = (b >= ny) + (b >= ny + nc);
    const short8 c = *reinterpret_cast<const short8*>(a.slot + (size_t)a.nf * sizeof(JpegFrameHdr) + blk * 128 + (size_t)r * 16);
    const ushort8 q = *reinterpret_cast<const ushort8*>(&hdr->quant[comp][r * 8]);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (int)c[k] * (int)q[k];
  }
  int* L = lds + lb * kLdsBlock;
#pragma unroll
  for (int k = 0; k < 8; ++k) L[r * 8 + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = L[k * 8 + r];   // column r
  idct_pass(v, t, 11);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) L[k * 8 + r] = t[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) v[k] = L[r * 8 + k];   // row r of the pass-1 result
  idct_pass(v, t, 18);
  if (live) {
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo |= (unsigned)clamp255(t[k] + 128) << (8 * k);
      hi |= (unsigned)clamp255(t[4 + k] + 128) << (8 * k);
    }
    *reinterpret_cast<uint2*>(a.planes + blk * 64 + (size_t)r * 8) = make_uint2(lo, hi);
  }
}

// ---- upsampling + colour ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ size_t smp_at(int bw, int y, int x) { return ((size_t)(y >> 3) * bw + (size_t)(x >> 3)) * 64 + (size_t)((y & 7) * 8 + (x & 7)); }

struct ChromaGeom { int bw, mode, fancy, dw, dh; };

// One chroma sample at full resolution.  Fancy h2v1: (3 p[i] + p[i -/+ 1] + 1 / 2) >> 2; fancy h2v2: t = 3 p[r] + p[r -/+ 1]
// vertically, then (3 t[i] + t[i -/+ 1] + 8 / 7) >> 4; the neighbour index clamped into the plane gives libjpeg's edge
// columns and rows, the neighbour replaced by the sample itself gives its plain replication.
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ P, const ChromaGeom& g, int y, int x) {
  if (g.mode == ST_JPEG_444) return P[smp_at(g.bw, y, x)];
  const int i = x >> 1;
  int j = i + ((x & 1) ? 1 : -1);
  j = j < 0 ? 0 : (j > g.dw - 1 ? g.dw - 1 : j);
  if (!g.fancy) j = i;
  if (g.mode == ST_JPEG_H2V1) return (3 * P[smp_at(g.bw, y, i)] + P[smp_at(g.bw, y, j)] + ((x & 1) ? 2 : 1)) >> 2;
  const int r = y >> 1;
  int r2 = r + ((y & 1) ? 1 : -1);
  r2 = r2 < 0 ? 0 : (r2 > g.dh - 1 ? g.dh - 1 : r2);
  if (!g.fancy) r2 = r;
  const int ti = 3 * P[smp_at(g.bw, r, i)] + P[smp_at(g.bw, r2, i)];
  const int tj = 3 * P[smp_at(g.bw, r, j)] + P[smp_at(g.bw, r2, j)];
  return (3 * ti + tj + ((x & 1) ? 7 : 8)) >> 4;
}

__device__ __forceinline__ void unpack8(uint2 v, int* o) {
#pragma unroll
  for (int k = 0; k < 4; ++k) { o[k] = (v.x >> (8 * k)) & 0xff; o[4 + k] = (v.y >> (8 * k)) & 0xff; }
}

// 16 chroma samples of output columns x0 .. x0 + 15 (x0 a multiple of 16, the row 16-sample aligned: w % 16 == 0, so dw is a
// multiple of 8 above 2 and the filter is always the fancy one): per source row one 8-byte block row and its two neighbours.
__device__ __forceinline__ void chroma16(const uint8_t* __restrict__ P, const ChromaGeom& g, int y, int x0, int* o) {
  if (g.mode == ST_JPEG_444) {
    unpack8(*reinterpret_cast<const uint2*>(P + smp_at(g.bw, y, x0)), o);
    unpack8(*reinterpret_cast<const uint2*>(P + smp_at(g.bw, y, x0 + 8)), o + 8);
    return;
  }
  const int i0 = x0 >> 1;
  const int il = i0 > 0 ? i0 - 1 : 0, ir = i0 + 8 < g.dw ? i0 + 8 : g.dw - 1;
  int s[10];
  if (g.mode == ST_JPEG_H2V1) {
    unpack8(*reinterpret_cast<const uint2*>(P + smp_at(g.bw, y, i0)), s + 1);
    s[0] = P[smp_at(g.bw, y, il)];
    s[9] = P[smp_at(g.bw, y, ir)];
#pragma unroll
    for (int p = 0; p < 16; ++p) o[p] = (3 * s[1 + (p >> 1)] + s[1 + (p >> 1) + ((p & 1) ? 1 : -1)] + ((p & 1) ? 2 : 1)) >> 2;
    return;
  }
  const int r = y >> 1;
  int r2 = r + ((y & 1) ? 1 : -1);
  r2 = r2 < 0 ? 0 : (r2 > g.dh - 1 ? g.dh - 1 : r2);
  int u[10];
  unpack8(*reinterpret_cast<const uint2*>(P + smp_at(g.bw, r, i0)), s + 1);
  s[0] = P[smp_at(g.bw, r, il)];
  s[9] = P[smp_at(g.bw, r, ir)];
  unpack8(*reinterpret_cast<const uint2*>(P + smp_at(g.bw, r2, i0)), u + 1);
  u[0] = P[smp_at(g.bw, r2, il)];
  u[9] = P[smp_at(g.bw, r2, ir)];
#pragma unroll
  for (int k = 0; k < 10; ++k) s[k] = 3 * s[k] + u[k];
#pragma unroll
  for (int p = 0; p < 16; ++p) o[p] = (3 * s[1 + (p >> 1)] + s[1 + (p >> 1) + ((p & 1) ? 1 : -1)] + ((p & 1) ? 7 : 8)) >> 4;
}

// PX pixels of one row per thread.  PX = 16: w % 16 == 0 and 16-byte aligned frames, whole 16-byte stores (three per thread, one
// for a one-component frame); PX = 4: w % 4 == 0 and 4-byte aligned frames, dword stores; PX = 1: anything, byte stores.
template <int PX>
__global__ __launch_bounds__(256) void k_jpeg_color(JpegArgsK a) {
  const JpegFrameHdr* __restrict__ hdr = reinterpret_cast<const JpegFrameHdr*>(a.slot) + blockIdx.y;
  const uint8_t* __restrict__ PY = a.planes + (size_t)hdr->blk_off * 64;
  const uint8_t* __restrict__ PB = PY + (size_t)hdr->nblk_y * 64;
  const uint8_t* __restrict__ PR = PB + (size_t)hdr->nblk_c * 64;
  const int bwy = hdr->bw_y;
  ChromaGeom g;
  g.bw = hdr->bw_c; g.mode = hdr->mode; g.fancy = hdr->fancy; g.dw = hdr->dw; g.dh = hdr->dh;
  uint8_t* __restrict__ out = st_gl(hdr->out);
  const int w = a.w, cn = a.channels;
  const long long groups = (long long)a.h * w / PX;
  for (long long gi = (long long)blockIdx.x * 256 + threadIdx.x; gi < groups; gi += (long long)gridDim.x * 256) {
    const long long pix = gi * PX;
    const int y = (int)(pix / w), x0 = (int)(pix % w);
    int Y[PX], Cb[PX], Cr[PX];
    if constexpr (PX == 16) {
      unpack8(*reinterpret_cast<const uint2*>(PY + smp_at(bwy, y, x0)), Y);
      unpack8(*reinterpret_cast<const uint2*>(PY + smp_at(bwy, y, x0 + 8)), Y + 8);
      if (cn == 3) {
        chroma16(PB, g, y, x0, Cb);
        chroma16(PR, g, y, x0, Cr);
      }
    } else {
#pragma unroll
      for (int p = 0; p < PX; ++p) {
        Y[p] = PY[smp_at(bwy, y, x0 + p)];
        if (cn == 3) {
          Cb[p] = chroma_at(PB, g, y, x0 + p);
          Cr[p] = chroma_at(PR, g, y, x0 + p);
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

// ---- host ---------------------------------------------------------------------------------------------------------------
struct SubBatch : StPipeSubBatch { size_t blocks; };

int jpeg_threads(int n) { return st_pipe_threads("ST_JPEG_THREADS", n); }

// the header the two dense kernels read, from a parsed stream; d: the scale denominator (1: full size)
void jpeg_frame_hdr(const StJpegHeader& hd, uint8_t* out, int blk_off, JpegFrameHdr* fh, int d) {
  memset(fh, 0, sizeof *fh);
  fh->out = out;
  fh->blk_off = blk_off;
  fh->nblk_y = (int)st_jpeg_comp_blocks(hd, 0);
  fh->nblk_c = hd.ncomp == 3 ? (int)st_jpeg_comp_blocks(hd, 1) : 0;
  fh->bw_y = hd.bw[0];
  fh->bw_c = hd.ncomp == 3 ? hd.bw[1] : 0;
  fh->mode = hd.mode;
  fh->dw = (hd.w + hd.hs[0] - 1) / hd.hs[0];
  fh->dh = (hd.h + hd.vs[0] - 1) / hd.vs[0];
  fh->fancy = fh->dw > 2 ? 1 : 0;
  if (d > 1) {
    // the reduced planes (st_jpeg_reduced.hip): what upsampling is left is h2v1, and libjpeg replicates at 1/8
    int S[3], dw[3], dh[3];
    st_jpeg_reduced_geom(hd, d, S, dw, dh);
    fh->s_y = S[0];
    fh->s_c = hd.ncomp == 3 ? S[1] : S[0];
    fh->ups = hd.ncomp == 3 ? hd.hs[0] * (8 / d) / S[1] : 1;
    fh->dw = hd.ncomp == 3 ? dw[1] : dw[0];
    fh->dh = hd.ncomp == 3 ? dh[1] : dh[0];
    fh->fancy = fh->ups == 2 && fh->dw > 2 && d < 8 ? 1 : 0;
  }
  for (int c = 0; c < hd.ncomp; ++c) memcpy(fh->quant[c], hd.quant[hd.tq[c]], 128);
}

// output pixels per lane of the colour kernels: 16 or 4 where the width written and every frame's address are multiples of it
int store_width(int ow, uint8_t* const* out_dev, int n) {
  unsigned align = 0;
  for (int i = 0; i < n; ++i) align |= (unsigned)(uintptr_t)out_dev[i];
  return (ow % 16 == 0 && (align & 15) == 0) ? 16 : ((ow % 4 == 0 && (align & 3) == 0) ? 4 : 1);
}

// what sizes the dense grids of a sub-batch: the most blocks any frame has, and the most of st_jpeg_reduced_counts
struct DenseMost { size_t most = 0, most1 = 0, mostlds = 0; };
DenseMost dense_most(const JpegFrameHdr* fh, int count) {
  DenseMost m;
  for (int j = 0; j < count; ++j) {
    m.most = std::max(m.most, (size_t)fh[j].nblk_y + 2 * (size_t)fh[j].nblk_c);
    size_t n1, nlds;
    st_jpeg_reduced_counts(fh[j], &n1, &nlds);
    m.most1 = std::max(m.most1, n1);
    m.mostlds = std::max(m.mostlds, nlds);
  }
  return m;
}

// the dense launches of nfl frames whose headers start at a.slot: the full-size pair, or the reduced ones
void launch_dense(st_ctx* ctx, JpegArgsK a, int nfl, int d, int px, const DenseMost& m) {
  if (d > 1) {
    a.h = (a.h + d - 1) / d;
    a.w = (a.w + d - 1) / d;
    st_jpeg_reduced_launch(ctx, a, nfl, m.most1, m.mostlds, px);
    return;
  }
  hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)((m.most + kIdctBlocks - 1) / kIdctBlocks), nfl), dim3(256), 0, ctx->stream, a);
  long long bx = ((long long)a.h * a.w / px + 255) / 256;
  if (bx > 8192) bx = 8192;
  const dim3 grid((unsigned)bx, nfl);
  if (px == 16) hipLaunchKernelGGL(k_jpeg_color<16>, grid, dim3(256), 0, ctx->stream, a);
  else if (px == 4) hipLaunchKernelGGL(k_jpeg_color<4>, grid, dim3(256), 0, ctx->stream, a);
  else hipLaunchKernelGGL(k_jpeg_color<1>, grid, dim3(256), 0, ctx->stream, a);
}

constexpr size_t kSlotCoefBytes = (size_t)64 << 20;   // coefficients of one sub-batch, unless a single frame has more

}  // namespace

struct st_jpeg_state {
  st_pinned_slots slots;   // of st_jpeg_decode_batch
  // st_jpeg_decode_batch_gpu: its one upload slot (the call waits for every sub-batch, so the slot is free when it is
  // refilled) and the page-locked words the status comes back in
  void* gpin = nullptr;
  size_t gcap = 0;
  void* gstatus = nullptr;
  size_t gstatus_cap = 0;
  int split_rounds = 0;   // st_jpeg_split_last_rounds
};

void st_jpeg_release(st_ctx* ctx) {
  if (!ctx->jpeg) return;
  st_slots_free(&ctx->jpeg->slots);
  if (ctx->jpeg->gpin) (void)hipHostFree(ctx->jpeg->gpin);
  if (ctx->jpeg->gstatus) (void)hipHostFree(ctx->jpeg->gstatus);
  delete ctx->jpeg;
  ctx->jpeg = nullptr;
}

namespace {
constexpr unsigned kJpegChannels = 1u << 1 | 1u << 3;

// ctx->jpeg, made at the first call
int jpeg_state(st_ctx* ctx, st_jpeg_state** js) {
  if (!ctx->jpeg) ctx->jpeg = new (std::nothrow) st_jpeg_state();
  if (!ctx->jpeg) return st_set_error(ctx, ST_ERR_OOM, "jpeg: out of host memory");
  *js = ctx->jpeg;
  return ST_OK;
}

// st_jpeg_decode_batch, the frames written at 1/d
int decode_batch_host(st_ctx* ctx, const uint8_t* const* bufs_host, const size_t* sizes, int n, int h, int w, int channels, uint8_t* const* out_dev,
                      const int d) {
  ST_TRY(st_decode_args(ctx, "jpeg", n, h, w, channels, kJpegChannels, bufs_host, sizes, out_dev));
  if (n == 0) return ST_OK;
  // every stream's markers first: nothing is launched or written unless all of them are streams this decodes, of one shape
  std::vector<StJpegHeader> hds((size_t)n);
  for (int i = 0; i < n; ++i) {
    char msg[160];
    if (!out_dev[i]) return st_set_error(ctx, ST_ERR_INVALID, kStNoOutputFrame, "jpeg", i);
    const int st = st_jpeg_parse_header(bufs_host[i], sizes[i], &hds[i], msg, sizeof msg);
    if (st != ST_OK) return st_set_error(ctx, st, "jpeg: stream %d: %s", i, msg);
    if (hds[i].h != h || hds[i].w != w || hds[i].ncomp != channels)
      return st_set_error(ctx, ST_ERR_INVALID, "jpeg: stream %d is %dx%d with %d channel(s), the call decodes %dx%d with %d", i, hds[i].w, hds[i].h,
                          hds[i].ncomp, w, h, channels);
  }
  const int T = jpeg_threads(n);
  std::vector<SubBatch> sbs;
  std::vector<int> blk_off((size_t)n);
  for (int i = 0; i < n; ++i) {
    const size_t nb = st_jpeg_blocks(hds[i]);
    if (sbs.empty() || sbs.back().count >= T || (sbs.back().blocks + nb) * 128 > kSlotCoefBytes) sbs.push_back(SubBatch{{i, 0}, 0});
    blk_off[i] = (int)sbs.back().blocks;
    sbs.back().count++;
    sbs.back().blocks += nb;
  }
  auto upload_bytes = [](const SubBatch& sb) { return (size_t)sb.count * sizeof(JpegFrameHdr) + sb.blocks * 128; };
  size_t slot_bytes = 0, plane_bytes = 0;
  for (const SubBatch& sb : sbs) {
    slot_bytes = std::max(slot_bytes, upload_bytes(sb));
    plane_bytes = std::max(plane_bytes, sb.blocks * 64);
  }
  st_jpeg_state* js;
  ST_TRY(jpeg_state(ctx, &js));
  st_pinned_slots* sl = &js->slots;
  ST_TRY(st_slots_prepare(ctx, sl, std::min(2, (int)sbs.size()), slot_bytes, "jpeg: cannot page-lock %zu bytes for the coefficients"));
  ST_TRY(st_ws_reserve(ctx, st_align_up(slot_bytes) + st_align_up(plane_bytes)));
  uint8_t* d_slot = (uint8_t*)st_ws_alloc(ctx, slot_bytes);
  uint8_t* d_planes = (uint8_t*)st_ws_alloc(ctx, plane_bytes);
  if (!d_slot || !d_planes) return st_set_error(ctx, ST_ERR_OOM, "jpeg: workspace exhausted");
  const int px = store_width((w + d - 1) / d, out_dev, n);

  // a stream's header and coefficients into its sub-batch's slot
  auto fill = [&](int i, int k, int s, char* msg, size_t msg_len) {
    JpegFrameHdr* fh = reinterpret_cast<JpegFrameHdr*>(sl->at(s)) + (i - sbs[k].first);
    jpeg_frame_hdr(hds[i], out_dev[i], blk_off[i], fh, d);
    int16_t* coef = reinterpret_cast<int16_t*>(sl->at(s) + (size_t)sbs[k].count * sizeof(JpegFrameHdr) + (size_t)blk_off[i] * 128);
    return st_jpeg_decode_scan(bufs_host[i], sizes[i], hds[i], coef, msg, msg_len);
  };
  // one copy and the dense launches
  auto issue = [&](int k, int s) -> int {
    const SubBatch& sb = sbs[k];
    ST_TRY(st_slot_upload(ctx, sl, s, d_slot, upload_bytes(sb)));
    JpegArgsK a;
    a.slot = d_slot; a.planes = d_planes; a.nf = sb.count; a.h = h; a.w = w; a.channels = channels;
    {
      st_timed t(ctx, ST_K_JPEG);
      launch_dense(ctx, a, sb.count, d, px, dense_most(reinterpret_cast<const JpegFrameHdr*>(sl->at(s)), sb.count));
    }
    ST_HIP(ctx, hipGetLastError());
    return ST_OK;
  };
  const StPipeResult r = st_pipe_run(sbs, T, fill, issue, [&](int s) { return st_slot_release(ctx, sl, s); });
  return r.stream >= 0 ? st_set_error(ctx, r.status, "jpeg: stream %d: %s", r.stream, r.message) : r.status;
}
}  // namespace

ST_EXPORT int st_jpeg_decode_batch(st_ctx* ctx, const uint8_t* const* bufs_host, const size_t* sizes, int n, int h, int w, int channels,
                                   uint8_t* const* out_dev) {
  ST_TRY(st_enter(ctx));
  return decode_batch_host(ctx, bufs_host, sizes, n, h, w, channels, out_dev, 1);
}

// ---- entropy decoding on the device -----------------------------------------------------------------------------------------
// The upload of a sub-batch of nf frames, one copy from the page-locked slot (every section 16-byte aligned):
//   [status word, 16 B] [table sets: StJpegFrameTables, one per run of frames with equal tables] [nf x StJpegEntFrame]
//   [interval tables: (begin, end) uint32 pairs relative to each frame's first entropy-coded byte]
//   [each frame's entropy-coded bytes from scan_pos, 16-byte aligned, padded by >= 16 zero bytes] [pad to 256]
//   [nf x JpegFrameHdr]
// and in device memory the sub-batch's coefficients follow the headers directly, so k_jpeg_idct finds them where it finds the
// uploaded ones of the host path (slot + nf * 512 + blk * 128).
namespace {

// Coefficients of one sub-batch, unless a single frame has more.  Device memory bounds it, not page-locked memory: the slot
// holds stream bytes only.  2 GiB keeps a 256-frame 1080p call (1.6 GB of coefficients, 17 408 restart intervals) ONE launch
// of one lane per interval; split further, each launch would have too few lanes to be worth it.
constexpr size_t kGpuCoefBytes = (size_t)2 << 30;

struct GpuStream {
  JpegFrameHdr fh;        // out and blk_off set when the sub-batches are laid out
  StJpegScanGeom geom;
  size_t scan_pos = 0, nbytes = 0, nblocks = 0;
  uint32_t nint = 0;
  int owner = 0;          // the scanning thread whose table holds this stream's intervals, at iv_at
  size_t iv_at = 0;
  bool same_tabs = false; // the tables equal those of the stream before it
  // its place in its sub-batch
  int sb = 0, tabs = 0;
  bool writes_tabs = false;
  size_t iv_off = 0, bytes_off = 0;
  // decoding by subsequence: its lanes, and where its prefix table of subsequence counts, its lanes and its segments start
  size_t nlanes = 0, subpre_off = 0, lane_off = 0, seg_off = 0;
};

struct GpuSubBatch {
  int first = 0, count = 0, nsets = 0;
  size_t blocks = 0, nint = 0;
  unsigned max_groups = 0;
  size_t tables_off = 0, frames_off = 0, hdr_off = 0, upload_bytes = 0;
  // decoding by subsequence: the StJsqFrame records in the upload, the lanes, and the per-lane state behind the coefficients
  size_t sq_off = 0, lanes = 0, scratch_off = 0;
  unsigned max_lane_groups = 0, max_segments = 0;
};

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

void frame_tables(const StJpegHeader& hd, StJpegFrameTables* t) {
  memset(t, 0, sizeof *t);
  for (int c = 0; c < hd.ncomp; ++c) {
    t->dc[c] = hd.dc[hd.td[c]];
    t->ac[c] = hd.ac[hd.ta[c]];
  }
}

template <class F>
void run_threads(int T, F&& f) {
  if (T <= 1) { f(0); return; }
  std::vector<std::thread> pool;
  pool.reserve((size_t)T);
  for (int t = 0; t < T; ++t) pool.emplace_back(f, t);
  for (std::thread& t : pool) t.join();
}

// A call of st_jpeg_decode_batch_gpu (split = false: one lane per restart interval) or st_jpeg_decode_batch_gpu_split (split =
// true: one lane per subsequence of S bytes, at most R round launches), which share everything but the entropy launches: its
// arguments, what the steps below make of them in turn, and the steps.
struct GpuPlan {
  st_ctx* ctx;
  const uint8_t* const* bufs_host;
  const size_t* sizes;
  int n, h, w, channels;
  uint8_t* const* out_dev;
  bool split;
  uint32_t S;
  int R, d, T;
  std::vector<GpuStream> gs;
  std::vector<std::vector<uint32_t>> ivs;   // the intervals (or segments) each scanning thread found
  std::vector<GpuSubBatch> sbs;
  size_t upload_most = 0, dev_most = 0, plane_most = 0;

  int probe_and_scan();
  void lay_out();
  int fill_slot(const GpuSubBatch& sb, uint8_t* slot) const;
  int run_sub_batch(const GpuSubBatch& sb, st_jpeg_state* js, uint8_t* d_up, uint8_t* d_planes, int px) const;
};

// 1. every stream's markers and its restart intervals, on T threads over contiguous runs of streams.  The lowest stream
// that is refused wins; only when none is, the lowest stream whose scan is broken.  Nothing is launched or written before.
int GpuPlan::probe_and_scan() {
  gs.resize((size_t)n);
  ivs.resize((size_t)T);
  struct Fail { int stream = INT_MAX, status = ST_OK; char msg[224]; };
  Fail probe_fail, scan_fail;
  std::mutex mu;
  auto note = [&](Fail& f, int i, int status, const char* fmt, auto... args) {
    std::lock_guard<std::mutex> lk(mu);
    if (i >= f.stream) return;
    f.stream = i;
    f.status = status;
    snprintf(f.msg, sizeof f.msg, fmt, args...);
  };
  try {
    run_threads(T, [&](int t) {
      const int lo = (int)((long long)n * t / T), hi = (int)((long long)n * (t + 1) / T);
      std::vector<StJpegHeader> hdv(1);
      std::vector<StJpegFrameTables> tv(2);
      StJpegHeader& hd = hdv[0];
      bool have_prev = false, scan_ok = true;
      char msg[160];
      for (int i = lo; i < hi; ++i) {
        GpuStream& g = gs[(size_t)i];
        if (!out_dev[i]) { note(probe_fail, i, ST_ERR_INVALID, kStNoOutputFrame, "jpeg", i); return; }
        const int st = st_jpeg_parse_header(bufs_host[i], sizes[i], &hd, msg, sizeof msg);
        if (st != ST_OK) { note(probe_fail, i, st, "jpeg: stream %d: %s", i, msg); return; }
        if (hd.h != h || hd.w != w || hd.ncomp != channels) {
          note(probe_fail, i, ST_ERR_INVALID, "jpeg: stream %d is %dx%d with %d channel(s), the call decodes %dx%d with %d", i, hd.w, hd.h, hd.ncomp, w, h, channels);
          return;
        }
        g.nint = (uint32_t)st_jpeg_interval_count(hd);
        if (g.nint == 0 && split) g.nint = 1;   // the whole scan is one segment
        if (g.nint == 0) {
          note(probe_fail, i, ST_ERR_UNSUPPORTED, "jpeg: stream %d: no restart intervals: the stream has no DRI segment, entropy decoding on the device needs one", i);
          return;
        }
        if (!scan_ok) continue;   // a later stream of this run may still be refused, which comes first
        jpeg_frame_hdr(hd, out_dev[i], 0, &g.fh, d);
        g.geom = st_jpeg_scan_geom(hd);
        g.scan_pos = hd.scan_pos;
        g.nblocks = st_jpeg_blocks(hd);
        frame_tables(hd, &tv[(size_t)(i & 1)]);
        g.same_tabs = have_prev && memcmp(&tv[0], &tv[1], sizeof(StJpegFrameTables)) == 0;
        have_prev = true;
        std::vector<uint32_t>& iv = ivs[(size_t)t];
        g.owner = t;
        g.iv_at = iv.size();
        iv.resize(iv.size() + 2 * (size_t)g.nint);
        const int ss = split ? st_jpeg_segments(bufs_host[i], sizes[i], hd, iv.data() + g.iv_at, msg, sizeof msg)
                             : st_jpeg_scan_intervals(bufs_host[i], sizes[i], hd, iv.data() + g.iv_at, msg, sizeof msg);
        if (ss != ST_OK) {
          note(scan_fail, i, ss, "jpeg: stream %d: %s", i, msg);
          scan_ok = false;
          continue;
        }
        g.nbytes = (size_t)iv[g.iv_at + 2 * (size_t)g.nint - 1] - g.scan_pos;
        if (split)
          for (size_t k = 0; k < g.nint; ++k) g.nlanes += st_jsq_count(iv[g.iv_at + 2 * k + 1] - iv[g.iv_at + 2 * k], S);
      }
    });
  } catch (const std::exception&) {
    return st_set_error(ctx, ST_ERR_OOM, "jpeg: out of host memory (or threads) for the interval tables");
  }
  if (probe_fail.stream != INT_MAX) return st_set_error(ctx, probe_fail.status, "%s", probe_fail.msg);
  if (scan_fail.stream != INT_MAX) return st_set_error(ctx, scan_fail.status, "%s", scan_fail.msg);
  return ST_OK;
}

// 2. sub-batches and the layout of each one's upload
void GpuPlan::lay_out() {
  auto close = [&]() {
    if (sbs.empty()) return;
    GpuSubBatch& sb = sbs.back();
    sb.tables_off = 16;
    sb.frames_off = up16(sb.tables_off + (size_t)sb.nsets * sizeof(StJpegFrameTables));
    size_t o = sb.frames_off + (size_t)sb.count * sizeof(StJpegEntFrame);
    if (split) { sb.sq_off = o; o += (size_t)sb.count * sizeof(StJsqFrame); }
    for (int i = sb.first; i < sb.first + sb.count; ++i) { gs[(size_t)i].iv_off = o; o += (size_t)gs[(size_t)i].nint * 8; }
    if (split)
      for (int i = sb.first; i < sb.first + sb.count; ++i) { gs[(size_t)i].subpre_off = o; o += ((size_t)gs[(size_t)i].nint + 1) * 4; }
    o = up16(o);
    for (int i = sb.first; i < sb.first + sb.count; ++i) { gs[(size_t)i].bytes_off = o; o += up16(gs[(size_t)i].nbytes + 16); }
    sb.hdr_off = st_align_up(o);
    sb.upload_bytes = sb.hdr_off + (size_t)sb.count * sizeof(JpegFrameHdr);
    upload_most = std::max(upload_most, sb.upload_bytes);
    // behind the coefficients: per lane two exit states, the entered-from state and four counts; per segment a flag; four
    // counters of changed exits
    sb.scratch_off = up16(sb.upload_bytes + sb.blocks * 128);
    dev_most = std::max(dev_most, split ? sb.scratch_off + sb.lanes * 40 + up16(sb.nint * 4) + 16 : sb.upload_bytes + sb.blocks * 128);
    plane_most = std::max(plane_most, sb.blocks * 64);
  };
  for (int i = 0; i < n; ++i) {
    GpuStream& g = gs[(size_t)i];
    if (sbs.empty() || (sbs.back().blocks + g.nblocks) * 128 > kGpuCoefBytes || sbs.back().lanes + g.nlanes > ((size_t)1 << 31) ||
        sbs.back().nint + g.nint > ((size_t)1 << 31)) {
      close();
      sbs.push_back(GpuSubBatch());
      sbs.back().first = i;
    }
    GpuSubBatch& sb = sbs.back();
    g.sb = (int)sbs.size() - 1;
    g.writes_tabs = sb.count == 0 || !g.same_tabs || gs[(size_t)i - 1].owner != g.owner;
    if (g.writes_tabs) sb.nsets++;
    g.tabs = sb.nsets - 1;
    g.fh.blk_off = (int)sb.blocks;
    g.lane_off = sb.lanes;
    g.seg_off = sb.nint;
    sb.lanes += g.nlanes;
    sb.max_lane_groups = std::max(sb.max_lane_groups, (unsigned)((g.nlanes + (size_t)kStJsqLanes - 1) / (size_t)kStJsqLanes));
    sb.max_segments = std::max(sb.max_segments, g.nint);
    sb.count++;
    sb.blocks += g.nblocks;
    sb.nint += g.nint;
    sb.max_groups = std::max(sb.max_groups, (g.nint + (unsigned)kStJpegEntLanes - 1) / (unsigned)kStJpegEntLanes);
  }
  close();
}

// 3. fill the slot on the threads (free: the previous sub-batch was waited for)
int GpuPlan::fill_slot(const GpuSubBatch& sb, uint8_t* slot) const {
  memset(slot, 0xFF, 16);   // the status word: clean
  std::atomic<int> next{sb.first};
  std::atomic<bool> bad{false};
  run_threads(std::min(T, sb.count), [&](int) {
    std::vector<StJpegHeader> hdv;
    char msg[160];
    for (;;) {
      const int i = next.fetch_add(1);
      if (i >= sb.first + sb.count) return;
      const GpuStream& g = gs[(size_t)i];
      const int j = i - sb.first;
      StJpegEntFrame* ef = reinterpret_cast<StJpegEntFrame*>(slot + sb.frames_off) + j;
      ef->geom = g.geom;
      ef->nint = g.nint;
      ef->tables = (uint32_t)g.tabs;
      ef->intervals_off = g.iv_off;
      ef->bytes_off = g.bytes_off;
      ef->nbytes = (uint32_t)g.nbytes;
      ef->blk_off = (uint32_t)g.fh.blk_off;
      if (g.writes_tabs) {
        if (hdv.empty()) hdv.resize(1);
        if (st_jpeg_parse_header(bufs_host[i], sizes[i], &hdv[0], msg, sizeof msg) != ST_OK) { bad = true; return; }   // the caller changed the stream
        frame_tables(hdv[0], reinterpret_cast<StJpegFrameTables*>(slot + sb.tables_off) + g.tabs);
      }
      const uint32_t* iv = ivs[(size_t)g.owner].data() + g.iv_at;
      uint32_t* dv = reinterpret_cast<uint32_t*>(slot + g.iv_off);
      for (size_t k = 0; k < 2 * (size_t)g.nint; ++k) dv[k] = iv[k] - (uint32_t)g.scan_pos;
      if (split) {
        StJsqFrame* qf = reinterpret_cast<StJsqFrame*>(slot + sb.sq_off) + j;
        memset(qf, 0, sizeof *qf);
        qf->subpre_off = g.subpre_off;
        qf->lane_off = (uint32_t)g.lane_off;
        qf->seg_off = (uint32_t)g.seg_off;
        qf->nlanes = (uint32_t)g.nlanes;
        uint32_t* pre = reinterpret_cast<uint32_t*>(slot + g.subpre_off);
        uint32_t sum = 0;
        for (size_t k = 0; k < g.nint; ++k) { pre[k] = sum; sum += st_jsq_count(iv[2 * k + 1] - iv[2 * k], S); }
        pre[g.nint] = sum;
      }
      memcpy(slot + g.bytes_off, bufs_host[i] + g.scan_pos, g.nbytes);
      memset(slot + g.bytes_off + g.nbytes, 0, up16(g.nbytes + 16) - g.nbytes);
      memcpy(slot + sb.hdr_off + (size_t)j * sizeof(JpegFrameHdr), &g.fh, sizeof(JpegFrameHdr));
    }
  });
  if (bad) return st_set_error(ctx, ST_ERR_INVALID, "jpeg: a stream changed during the call");
  return ST_OK;
}

// 4. one copy of the filled slot (js->gpin), the entropy launch, the ONE host wait of the sub-batch (its status word), then the
// dense kernels
int GpuPlan::run_sub_batch(const GpuSubBatch& sb, st_jpeg_state* js, uint8_t* d_up, uint8_t* d_planes, int px) const {
  unsigned long long* const gstatus = static_cast<unsigned long long*>(js->gstatus);
  unsigned long long word = kStJpegEntClean;
  {
    st_timed timed(ctx, ST_K_JPEG);
    ST_HIP(ctx, hipMemcpyAsync(d_up, js->gpin, sb.upload_bytes, hipMemcpyHostToDevice, ctx->stream));
    StJpegEntArgs ea;
    ea.upload = d_up;
    ea.frames = reinterpret_cast<const StJpegEntFrame*>(d_up + sb.frames_off);
    ea.tables = reinterpret_cast<const StJpegFrameTables*>(d_up + sb.tables_off);
    ea.coef = reinterpret_cast<int16_t*>(d_up + sb.upload_bytes);
    ea.status = reinterpret_cast<unsigned long long*>(d_up);
    ea.nf = sb.count;
    ea.first_stream = sb.first;
    if (!split) {
      ST_TRY(st_jpeg_entropy_launch(ctx, ea, sb.max_groups));
    } else {
      StJsqArgs qa;
      qa.ent = ea;
      qa.sq = reinterpret_cast<const StJsqFrame*>(d_up + sb.sq_off);
      uint8_t* scratch = d_up + sb.scratch_off;
      qa.exits[0] = reinterpret_cast<uint64_t*>(scratch + sb.lanes * 16);
      qa.exits[1] = reinterpret_cast<uint64_t*>(scratch + sb.lanes * 24);
      qa.entered = reinterpret_cast<uint64_t*>(scratch + sb.lanes * 32);
      qa.counts = reinterpret_cast<uint32_t*>(scratch);   // 16 bytes per lane, 16-byte aligned
      qa.unconverged = reinterpret_cast<uint32_t*>(scratch + sb.lanes * 40);
      qa.changed = reinterpret_cast<unsigned*>(scratch + sb.lanes * 40 + up16(sb.nint * 4));
      qa.S = S;
      // round launches in groups (three, then two at a time), one host wait per group for its counts of changed exits: a
      // launch that changed none has verified the chain.  Launches behind it in its group change nothing either.
      int launches = 0, rounds = R;
      bool converged = false;
      unsigned* back = reinterpret_cast<unsigned*>(gstatus + 1);
      while (launches < R && !converged) {
        const int group = std::min(launches == 0 ? 3 : 2, R - launches);
        ST_HIP(ctx, hipMemsetAsync(qa.changed, 0, 16, ctx->stream));
        for (int q = 0; q < group; ++q, ++launches) ST_TRY(st_jsq_round_launch(ctx, qa, sb.max_lane_groups, launches == 0, launches & 1, qa.changed + q));
        ST_HIP(ctx, hipMemcpyAsync(back, qa.changed, 16, hipMemcpyDeviceToHost, ctx->stream));
        ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int q = 0; q < group && !converged; ++q)
          if (back[q] == 0) { converged = true; rounds = launches - group + q; }
      }
      js->split_rounds = std::max(js->split_rounds, rounds);
      ST_TRY(st_jsq_finish_launch(ctx, qa, sb.max_lane_groups, sb.max_segments, (launches - 1) & 1, sb.blocks * 128));
    }
    ST_HIP(ctx, hipMemcpyAsync(gstatus, d_up, sizeof word, hipMemcpyDeviceToHost, ctx->stream));
    ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
    word = *gstatus;
    if (word == kStJpegEntClean) {
      const DenseMost m = dense_most(reinterpret_cast<const JpegFrameHdr*>(static_cast<const uint8_t*>(js->gpin) + sb.hdr_off), sb.count);
      // the dense kernels take the frame from blockIdx.y: the headers of a launch are offset so that the coefficients stay
      // where slot + nf * 512 points
      (void)st_for_launches(sb.count, [&](int f0, int nfl) -> int {
        JpegArgsK a;
        a.slot = d_up + sb.hdr_off + (size_t)f0 * sizeof(JpegFrameHdr);
        a.planes = d_planes; a.nf = sb.count - f0; a.h = h; a.w = w; a.channels = channels;
        launch_dense(ctx, a, nfl, d, px, m);
        return ST_OK;
      });
    }
  }
  ST_HIP(ctx, hipGetLastError());
  if (word != kStJpegEntClean) {
    const int stream = (int)(word >> 32);
    const unsigned interval = (unsigned)((word >> 4) & 0xfffffffu);
    const unsigned nint = stream >= 0 && stream < n ? gs[(size_t)stream].nint : 0u;
    if (split && stream >= 0 && stream < n && gs[(size_t)stream].geom.restart_interval <= 0)
      return st_set_error(ctx, ST_ERR_INVALID, "jpeg: stream %d: corrupt scan: the scan: %s", stream, st_jpeg_entropy_cause((int)(word & 15)));
    return st_set_error(ctx, ST_ERR_INVALID, "jpeg: stream %d: corrupt scan: restart interval %u of %u: %s", stream, interval, nint,
                        st_jpeg_entropy_cause((int)(word & 15)));
  }
  return ST_OK;
}

int decode_batch_gpu(st_ctx* ctx, const uint8_t* const* bufs_host, const size_t* sizes, int n, int h, int w, int channels, uint8_t* const* out_dev,
                     const bool split, const uint32_t S, const int R, const int d) {
  ST_TRY(st_decode_args(ctx, "jpeg", n, h, w, channels, kJpegChannels, bufs_host, sizes, out_dev));
  if (n == 0) return ST_OK;
  GpuPlan p{ctx, bufs_host, sizes, n, h, w, channels, out_dev, split, S, R, d, jpeg_threads(n)};
  ST_TRY(p.probe_and_scan());
  p.lay_out();
  st_jpeg_state* js;
  ST_TRY(jpeg_state(ctx, &js));
  ST_TRY(st_pinned_grow(ctx, &js->gstatus, &js->gstatus_cap, 64, "jpeg: cannot page-lock the status word"));
  // (an eighth more than this call needs, so that calls of slowly growing size do not each allocate again)
  if (p.upload_most > js->gcap)
    ST_TRY(st_pinned_grow(ctx, &js->gpin, &js->gcap, p.upload_most + p.upload_most / 8, "jpeg: cannot page-lock %zu bytes for the streams"));
  ST_TRY(st_ws_reserve(ctx, st_align_up(p.dev_most) + st_align_up(p.plane_most)));
  uint8_t* d_up = (uint8_t*)st_ws_alloc(ctx, p.dev_most);
  uint8_t* d_planes = (uint8_t*)st_ws_alloc(ctx, p.plane_most);
  if (!d_up || !d_planes) return st_set_error(ctx, ST_ERR_OOM, "jpeg: workspace exhausted");
  const int px = store_width((w + d - 1) / d, out_dev, n);
  for (const GpuSubBatch& sb : p.sbs) {
    ST_TRY(p.fill_slot(sb, static_cast<uint8_t*>(js->gpin)));
    ST_TRY(p.run_sub_batch(sb, js, d_up, d_planes, px));
  }
  return ST_OK;
}
}  // namespace

ST_EXPORT int st_jpeg_decode_batch_gpu(st_ctx* ctx, const uint8_t* const* bufs_host, const size_t* sizes, int n, int h, int w, int channels,
                                       uint8_t* const* out_dev) {
  ST_TRY(st_enter(ctx));
  return decode_batch_gpu(ctx, bufs_host, sizes, n, h, w, channels, out_dev, false, 0, 0, 1);
}

namespace {
int decode_batch_split(st_ctx* ctx, const uint8_t* const* bufs_host, const size_t* sizes, int n, int h, int w, int channels, uint8_t* const* out_dev,
                       const st_jpeg_split_opts* opts, const int d) {
  const int S = opts && opts->subseq_bytes ? opts->subseq_bytes : kStJsqDefaultSubseqBytes;
  const int R = opts && opts->max_rounds ? opts->max_rounds : kStJsqDefaultMaxRounds;
  if (S < 8 || S > 4096 || S % 8 != 0 || R < 0)
    return st_set_error(ctx, ST_ERR_INVALID, "jpeg: subseq_bytes %d / max_rounds %d: a multiple of 8 in 8..4096, and no negative cap", S, R);
  if (ctx->jpeg) ctx->jpeg->split_rounds = 0;
  return decode_batch_gpu(ctx, bufs_host, sizes, n, h, w, channels, out_dev, true, (uint32_t)S, R, d);
}
}  // namespace

ST_EXPORT int st_jpeg_decode_batch_gpu_split(st_ctx* ctx, const uint8_t* const* bufs_host, const size_t* sizes, int n, int h, int w, int channels,
                                             uint8_t* const* out_dev, const st_jpeg_split_opts* opts) {
  ST_TRY(st_enter(ctx));
  return decode_batch_split(ctx, bufs_host, sizes, n, h, w, channels, out_dev, opts, 1);
}

ST_EXPORT int st_jpeg_decode_batch_scaled(st_ctx* ctx, const uint8_t* const* bufs_host, const size_t* sizes, int n, int h, int w, int channels,
                                          int scale_denom, int entropy, const st_jpeg_split_opts* opts, uint8_t* const* out_dev) {
  ST_TRY(st_enter(ctx));
  const int d = scale_denom;
  if (d != 1 && d != 2 && d != 4 && d != 8) return st_set_error(ctx, ST_ERR_INVALID, "jpeg: scale_denom %d: 1, 2, 4 or 8", d);
  switch (entropy) {
    case ST_JPEG_ENTROPY_HOST: return decode_batch_host(ctx, bufs_host, sizes, n, h, w, channels, out_dev, d);
    case ST_JPEG_ENTROPY_INTERVAL: return decode_batch_gpu(ctx, bufs_host, sizes, n, h, w, channels, out_dev, false, 0, 0, d);
    case ST_JPEG_ENTROPY_SUBSEQUENCE: return decode_batch_split(ctx, bufs_host, sizes, n, h, w, channels, out_dev, opts, d);
  }
  return st_set_error(ctx, ST_ERR_INVALID, "jpeg: entropy %d: ST_JPEG_ENTROPY_HOST (0), _INTERVAL (1) or _SUBSEQUENCE (2)", entropy);
}

ST_EXPORT int st_jpeg_split_last_rounds(st_ctx* ctx) { return ctx && ctx->jpeg ? ctx->jpeg->split_rounds : 0; }
