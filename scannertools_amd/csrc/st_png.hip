// ImageDecoder, PNG: the streams are inflated on host threads (st_png_host.cpp), the row filters are undone and the frames
// expanded here.  DESIGN.md 4.17.
//
// k_png_unfilter: ONE workgroup of one wave per frame.  The filters make every byte depend on its left, upper and upper-left
// neighbours, and Average and Paeth are not linear, so the rows of a frame are a skewed wavefront: lane l owns row
// band * 64 + l and trails lane l - 1 by one 16-byte piece.  The upper piece comes from the lane above by a cross-lane move
// (its output of the step before), the upper-left bytes are the tail of the upper piece of the step before, the left bytes the
// tail of the lane's own last piece: both stay in registers.  Lane 0's upper row is the last row of the band before, which the
// same wave stored: it drains its stores (vmcnt(0)) and passes a barrier before the next band, and reads that row past L1.
// k_png_expand: elementwise, for the frames whose layout is not the scanlines' (palette, depth < 8, gray + alpha, RGB + tRNS).
#include <algorithm>
#include <cstring>
#include <new>

#include "st_host_pipeline.h"
#include "st_internal.h"
#include "st_png_host.h"

namespace {

// what the kernels read of a frame; nf of them head a sub-batch's upload slot
struct alignas(16) PngFrameHdr {
  uint8_t* out;                  // the (h, w, channels) frame
  unsigned long long data_off;   // of the frame's h x (1 + rowbytes) inflated bytes from the slot's start; 16 readable bytes follow them
  unsigned long long plane_off;  // of its h x rowbytes reconstructed bytes in the planes, unless kind is ST_PNG_DIRECT
  int h, w, bpp, rowbytes, kind, depth, channels;
  uint8_t key[4];
  uint8_t pal[1024];             // R, G, B, A by index
};
static_assert(sizeof(PngFrameHdr) % 16 == 0, "headers keep the data 16-byte aligned");

struct PngArgsK {
  const uint8_t* slot;
  uint8_t* planes;
  int nf;
};

typedef unsigned u32u __attribute__((aligned(1)));

__device__ __forceinline__ unsigned png_byte(const unsigned (&v)[4], int k) { return (v[k >> 2] >> (8 * (k & 3))) & 0xffu; }

// One 16-byte piece of a row.  x: the filtered bytes; b: the row above; left / ul: the last BPP bytes of this row's and of
// the upper row's piece before (zero in a row's first piece); both are moved on.  Bytes past the row's end come out as
// garbage that nothing reads.
template <int BPP>
__device__ __forceinline__ void png_piece(const unsigned (&x)[4], const unsigned (&b)[4], unsigned (&left)[BPP], unsigned (&ul)[BPP], int ft,
                                          unsigned (&o)[4]) {
  unsigned ob[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int xv = (int)png_byte(x, k), bv = (int)png_byte(b, k);
    const int av = (int)(k < BPP ? left[k < BPP ? k : 0] : ob[k < BPP ? 0 : k - BPP]);
    const int cv = (int)(k < BPP ? ul[k < BPP ? k : 0] : png_byte(b, k < BPP ? 0 : k - BPP));
    // Paeth: the distances of p = a + b - c, ties to a, then b, then c
    const int pa = abs(bv - cv), pb = abs(av - cv), pc = abs(av + bv - 2 * cv);
    const int pae = (pa <= pb && pa <= pc) ? av : (pb <= pc ? bv : cv);
    const int pred = ft == 1 ? av : ft == 2 ? bv : ft == 3 ? ((av + bv) >> 1) : ft == 4 ? pae : 0;
    ob[k] = (unsigned)(xv + pred) & 0xffu;
  }
#pragma unroll
  for (int k = 0; k < BPP; ++k) {
    left[k] = ob[16 - BPP + k];
    ul[k] = png_byte(b, 16 - BPP + k);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) o[q] = ob[4 * q] | ob[4 * q + 1] << 8 | ob[4 * q + 2] << 16 | ob[4 * q + 3] << 24;
}

__device__ __forceinline__ void png_load16(const uint8_t* p, unsigned (&v)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = reinterpret_cast<const u32u*>(p)[q];
}

// the carried row, read past L1 (nt): the line may sit there from before this wave rewrote it.  n: the bytes that exist
__device__ __forceinline__ void png_load_carry(const uint8_t* p, int n, unsigned (&v)[4]) {
  if (n >= 16) {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = __builtin_nontemporal_load(reinterpret_cast<const u32u*>(p) + q);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = 0;
#pragma unroll
    for (int k = 0; k < 15; ++k)   // (constant indices: the pieces stay in registers)
      if (k < n) v[k >> 2] |= (unsigned)__builtin_nontemporal_load(p + k) << (8 * (k & 3));
  }
}

template <int BPP>
__device__ void png_unfilter_frame(const uint8_t* __restrict__ raw, uint8_t* dst, const int h, const int rb) {
  const int lane = (int)threadIdx.x;
  const int nch = (rb + 15) >> 4;
  for (int band = 0; band * 64 < h; ++band) {
    const int row = band * 64 + lane;
    const bool rowok = row < h;
    const uint8_t* x = raw + (size_t)(rowok ? row : band * 64) * (size_t)(1 + rb);
    const int ft = rowok ? (int)x[0] : 0;
    x += 1;
    uint8_t* o = dst + (size_t)(rowok ? row : band * 64) * (size_t)rb;
    const bool carry = lane == 0 && band > 0;
    const uint8_t* upg = dst + (size_t)(band > 0 ? band * 64 - 1 : 0) * (size_t)rb;   // lane 0's upper row
    unsigned outc[4] = {0u, 0u, 0u, 0u}, xn[4] = {0u, 0u, 0u, 0u}, bn[4] = {0u, 0u, 0u, 0u};
    unsigned left[BPP], ul[BPP];
#pragma unroll
    for (int k = 0; k < BPP; ++k) left[k] = ul[k] = 0u;
    // every piece is fetched one step ahead of its use
    if (lane == 0) {
      png_load16(x, xn);
      if (carry) png_load_carry(upg, rb, bn);
    }
    for (int t = 0; t < nch + 63; ++t) {
      const int j = t - lane;
      unsigned b[4], xc[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        b[q] = __shfl_up(outc[q], 1);   // the lane above finished this piece in the step before
        xc[q] = xn[q];
      }
      if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = bn[q];   // zero in the frame's first row
      }
      const int jn = j + 1;
      if (rowok && jn >= 0 && jn < nch) {
        png_load16(x + 16 * jn, xn);   // up to 15 bytes past the row: the next row's, or the slot's padding
        if (carry) png_load_carry(upg + 16 * jn, rb - 16 * jn, bn);
      }
      if (rowok && j >= 0 && j < nch) {
        png_piece<BPP>(xc, b, left, ul, ft, outc);
        uint8_t* d = o + 16 * j;
        if (16 * j + 16 <= rb) {
#pragma unroll
          for (int q = 0; q < 4; ++q) reinterpret_cast<u32u*>(d)[q] = outc[q];
        } else {
#pragma unroll
          for (int k = 0; k < 15; ++k)
            if (k < rb - 16 * j) d[k] = (uint8_t)(outc[k >> 2] >> (8 * (k & 3)));
        }
      }
    }
    // the band's last row is the next band's upper row: its stores have left this wave (vmcnt(0)) before any lane reads it
    __threadfence_block();
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void k_png_unfilter(PngArgsK a) {
  const PngFrameHdr* fh = reinterpret_cast<const PngFrameHdr*>(a.slot) + blockIdx.y;
  const int h = fh->h, rb = fh->rowbytes, bpp = fh->bpp;
  const uint8_t* raw = a.slot + fh->data_off;
  uint8_t* dst = fh->kind == ST_PNG_DIRECT ? fh->out : a.planes + fh->plane_off;
  raw = st_gl(raw);
  dst = st_gl(dst);
  if (bpp == 1) png_unfilter_frame<1>(raw, dst, h, rb);
  else if (bpp == 2) png_unfilter_frame<2>(raw, dst, h, rb);
  else if (bpp == 3) png_unfilter_frame<3>(raw, dst, h, rb);
  else png_unfilter_frame<4>(raw, dst, h, rb);
}

__global__ __launch_bounds__(256) void k_png_expand(PngArgsK a) {
  const PngFrameHdr* fh = reinterpret_cast<const PngFrameHdr*>(a.slot) + blockIdx.y;
  const int kind = fh->kind;
  if (kind == ST_PNG_DIRECT) return;
  const int h = fh->h, w = fh->w, rb = fh->rowbytes, depth = fh->depth, ch = fh->channels;
  const uint8_t* __restrict__ pl = st_gl(a.planes + fh->plane_off);
  uint8_t* out = st_gl(fh->out);
  const uint8_t* pal = fh->pal;
  const unsigned k0 = fh->key[0], k1 = fh->key[1], k2 = fh->key[2];
  const int scale = depth == 1 ? 255 : depth == 2 ? 85 : depth == 4 ? 17 : 1;
  const long long npx = (long long)h * w;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npx; i += (long long)gridDim.x * 256) {
    const int y = (int)(i / w), xq = (int)(i - (long long)y * w);
    const uint8_t* r = pl + (size_t)y * rb;
    uint8_t* o = out + i * ch;
    if (kind == ST_PNG_GRAY_ALPHA) {
      const uint8_t g = r[2 * xq];
      o[0] = g; o[1] = g; o[2] = g; o[3] = r[2 * xq + 1];
    } else if (kind == ST_PNG_RGB_KEY) {
      const unsigned R = r[3 * xq], G = r[3 * xq + 1], B = r[3 * xq + 2];
      o[0] = (uint8_t)R; o[1] = (uint8_t)G; o[2] = (uint8_t)B;
      o[3] = (R == k0 && G == k1 && B == k2) ? 0 : 255;
    } else {
      const int bit = xq * depth;   // samples are packed from the most significant bit down
      const int v = depth == 8 ? r[xq] : (r[bit >> 3] >> (8 - depth - (bit & 7))) & ((1 << depth) - 1);
      if (kind == ST_PNG_GRAY_BITS) o[0] = (uint8_t)(v * scale);
      else for (int k = 0; k < ch; ++k) o[k] = pal[4 * v + k];
    }
  }
}

struct PngSubBatch : StPipeSubBatch { size_t data, planes; };
// Inflated bytes of one sub-batch, unless a single frame has more: sixteen 1080p RGBA frames.  A frame is one wave, so a
// sub-batch's unfilter launch takes as long as its slowest frame however many frames it has: at 64 MB (ten 1080p RGB frames) a
// 256-stream call made 26 launches of 20 ms and the device was as busy as the inflating threads; at sixteen it makes 16.
constexpr size_t kSlotDataBytes = (size_t)160 << 20;
inline size_t pad16(size_t v) { return (v + 15) / 16 * 16 + 16; }   // 16-byte aligned, and 16 bytes a piece may read past the end

}  // namespace

struct st_png_state { st_pinned_slots slots; };

void st_png_release(st_ctx* ctx) {
  if (!ctx->png) return;
  st_slots_free(&ctx->png->slots);
  delete ctx->png;
  ctx->png = nullptr;
}

ST_EXPORT int st_png_decode_batch(st_ctx* ctx, const uint8_t* const* bufs_host, const size_t* sizes, int n, int h, int w, int channels,
                                  uint8_t* const* out_dev) {
  ST_TRY(st_enter(ctx));
  ST_TRY(st_decode_args(ctx, "png", n, h, w, channels, 1u << 1 | 1u << 3 | 1u << 4, bufs_host, sizes, out_dev));
  if (n == 0) return ST_OK;
  // every stream's container first: nothing is launched or written unless all of them are streams this decodes, of one shape
  std::vector<StPngHeader> hds((size_t)n);
  for (int i = 0; i < n; ++i) {
    char msg[160];
    if (!out_dev[i]) return st_set_error(ctx, ST_ERR_INVALID, kStNoOutputFrame, "png", i);
    const int st = st_png_parse(bufs_host[i], sizes[i], true, &hds[i], msg, sizeof msg);
    if (st != ST_OK) return st_set_error(ctx, st, "png: stream %d: %s", i, msg);
    if (hds[i].h != h || hds[i].w != w || hds[i].channels != channels)
      return st_set_error(ctx, ST_ERR_INVALID, "png: stream %d is %dx%d with %d channel(s), the call decodes %dx%d with %d", i, hds[i].w, hds[i].h,
                          hds[i].channels, w, h, channels);
  }
  const int T = st_pipe_threads("ST_PNG_THREADS", n);
  std::vector<PngSubBatch> sbs;
  std::vector<size_t> data_off((size_t)n), plane_off((size_t)n);
  for (int i = 0; i < n; ++i) {
    const size_t nb = pad16(st_png_raw_bytes(hds[i]));
    if (sbs.empty() || sbs.back().count >= T || sbs.back().data + nb > kSlotDataBytes) sbs.push_back(PngSubBatch{{i, 0}, 0, 0});
    data_off[i] = sbs.back().data;
    plane_off[i] = sbs.back().planes;
    sbs.back().count++;
    sbs.back().data += nb;
    if (hds[i].kind != ST_PNG_DIRECT) sbs.back().planes += pad16((size_t)hds[i].h * hds[i].rowbytes);
  }
  auto upload_bytes = [](const PngSubBatch& sb) { return (size_t)sb.count * sizeof(PngFrameHdr) + sb.data; };
  size_t slot_bytes = 0, plane_bytes = 16;
  for (const PngSubBatch& sb : sbs) {
    slot_bytes = std::max(slot_bytes, upload_bytes(sb));
    plane_bytes = std::max(plane_bytes, sb.planes);
  }
  if (!ctx->png) ctx->png = new (std::nothrow) st_png_state();
  if (!ctx->png) return st_set_error(ctx, ST_ERR_OOM, "png: out of host memory");
  st_pinned_slots* sl = &ctx->png->slots;
  ST_TRY(st_slots_prepare(ctx, sl, std::min(2, (int)sbs.size()), slot_bytes, "png: cannot page-lock %zu bytes for the scanlines"));
  ST_TRY(st_ws_reserve(ctx, st_align_up(slot_bytes) + st_align_up(plane_bytes)));
  uint8_t* d_slot = (uint8_t*)st_ws_alloc(ctx, slot_bytes);
  uint8_t* d_planes = (uint8_t*)st_ws_alloc(ctx, plane_bytes);
  if (!d_slot || !d_planes) return st_set_error(ctx, ST_ERR_OOM, "png: workspace exhausted");

  // a stream's header and its inflated scanlines into its sub-batch's slot
  auto fill = [&](int i, int k, int s, char* msg, size_t msg_len) {
    const StPngHeader& hd = hds[i];
    PngFrameHdr* fh = reinterpret_cast<PngFrameHdr*>(sl->at(s)) + (i - sbs[k].first);
    memset(fh, 0, sizeof *fh);
    fh->out = out_dev[i];
    fh->data_off = (size_t)sbs[k].count * sizeof(PngFrameHdr) + data_off[i];
    fh->plane_off = plane_off[i];
    fh->h = hd.h; fh->w = hd.w; fh->bpp = hd.bpp; fh->rowbytes = hd.rowbytes; fh->kind = hd.kind; fh->depth = hd.bit_depth;
    fh->channels = hd.channels;
    memcpy(fh->key, hd.key, 3);
    memcpy(fh->pal, hd.pal, sizeof fh->pal);
    uint8_t* raw = sl->at(s) + fh->data_off;
    const int st = st_png_inflate_rows(bufs_host[i], hd, raw, msg, msg_len);
    memset(raw + st_png_raw_bytes(hd), 0, pad16(st_png_raw_bytes(hd)) - st_png_raw_bytes(hd));
    return st;
  };
  // one copy, the unfilter launch and, where a frame's layout is not the scanlines', the expansion
  auto issue = [&](int k, int s) -> int {
    const PngSubBatch& sb = sbs[k];
    ST_TRY(st_slot_upload(ctx, sl, s, d_slot, upload_bytes(sb)));
    PngArgsK a;
    a.slot = d_slot; a.planes = d_planes; a.nf = sb.count;
    {
      st_timed t(ctx, ST_K_JPEG);
      hipLaunchKernelGGL(k_png_unfilter, dim3(1, (unsigned)sb.count), dim3(64), 0, ctx->stream, a);
    }
    if (sb.planes) {
      long long bx = ((long long)h * w + 255) / 256;
      if (bx > 4096) bx = 4096;
      st_timed t(ctx, ST_K_JPEG);
      hipLaunchKernelGGL(k_png_expand, dim3((unsigned)bx, (unsigned)sb.count), dim3(256), 0, ctx->stream, a);
    }
    ST_HIP(ctx, hipGetLastError());
    return ST_OK;
  };
  const StPipeResult r = st_pipe_run(sbs, T, fill, issue, [&](int s) { return st_slot_release(ctx, sl, s); });
  return r.stream >= 0 ? st_set_error(ctx, r.status, "png: stream %d: %s", r.stream, r.message) : r.status;
}
