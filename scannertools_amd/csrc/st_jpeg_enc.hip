// ImageEncoder op, baseline JPEG: st_jpeg_encode_batch / st_jpeg_encode_fetch and their kernels.
//
// Resident (h, w, 3) uint8 frames become the streams libjpeg(-turbo) writes for them at the same quality and sampling with
// one restart interval per MCU row (include/scannertools_hip.h), byte for byte.  Everything runs on the GPU;
// only the finished streams cross to the host.  Four launches per call, no waiting between workgroups:
//   k_jpeg_fdct     one thread per 8 x 8 block: jccolor's RGB -> YCbCr, jcsample's h2v1 / h2v2 box filter with its
//                   alternating bias, the edge replication, jfdctint's forward DCT and the quantisation, all in registers;
//                   int16 coefficients in zigzag order, blocks in MCU order (padding blocks included), to the workspace
//   k_jpeg_entropy  one wave per restart interval, 64 blocks at a time: each lane measures its block's code length, a wave
//                   prefix sum places the blocks, the lanes OR their codes into a bit buffer in LDS (words on block
//                   boundaries are shared, hence ds_or), a second prefix sum over the 0xFF bytes places the stuffed zeros; the
//                   bytes go to the interval's slot, its length to a table.  A slot has the proven worst-case size
//                   (st_jpeg_enc_host.h: 416 bytes per block), so no interval depends on another's length.
//   k_jpeg_layout   one workgroup: every interval's offset in its stream (header, lengths, + 2 per RST marker), every
//                   stream's size, and the exclusive scan of the sizes = each stream's offset in the packed buffer
//   k_jpeg_pack     one workgroup per interval: copies the header (the frame's first interval), the interval's bytes and the
//                   marker that follows them (RSTn, or EOI after the last) to their place
// The header (SOI .. SOS) and the Huffman code tables are built on the host once per (h, w, quality, sampling, restart mode)
// and uploaded.
//
// st_jpeg_encode_batch_rst(..., ST_JPEG_RESTART_NONE) writes the stream without DRI and RSTn in five launches,
// again with no waiting between workgroups:
//   k_jpeg_fdct             as above
//   k_jpeg_entropy<false>   one wave per MCU row: DC predecessors from the row above, no padding, no stuffing; the row's bits
//                           and its length in bits
//   k_jpeg_ff_count         one workgroup per MCU row: its bit offset in the frame's scan, the bytes it owns (those whose first
//                           bit lies in it) and how many of them are 0xFF
//   k_jpeg_layout<false>    as above over the rows' stuffed lengths, nothing between rows, EOI at the end
//   k_jpeg_pack_bits        one workgroup per MCU row: header, the owned bytes shifted into place, completed from the next row
//                           (or with 1-bits) and stuffed, EOI
//
// st_jpeg_encode_batch_opt(..., optimize = 1) codes each frame with Huffman tables built from its own symbol counts, libjpeg's
// optimize_coding: two launches more, between the transform and the entropy coder, and no host wait:
//   k_jpeg_sym_stats        one wave per MCU row walks each block once and counts the symbols code_block will emit, per frame
//   k_jpeg_opt_tables       one workgroup per frame, one wave per table: jpeg_gen_optimal_table (st_jpeg_enc_opt.h), the frame's
//                           code words, its four DHT segments in its own header, the header's length
// The kernels above then run as their <.., OPT = true> instances: the frame's table and header instead of the call's, 1665 bits
// per block instead of 1660, and for streams without markers the ownership rule for rows as short as 6 bits (following_bits()).
// With optimize = 0 the <.., false> instances run, which are the kernels as they were.
#include <climits>
#include <cstring>
#include <vector>

#include "st_internal.h"
#include "st_jpeg_enc_host.h"
#include "st_jpeg_enc_opt.h"

struct st_jpeg_enc_state {
  // device: the header bytes at 0, the Huffman code words at kParamsHuff; what they were built for
  uint8_t* params = nullptr;
  int key[6] = {0, 0, 0, 0, 0, 0};   // h, w, quality, sampling, restart mode
  std::vector<uint8_t> params_host;
  // the streams of the last st_jpeg_encode_batch call, packed one after the other, and their n + 1 offsets
  uint8_t* blob = nullptr;
  size_t blob_cap = 0;
  unsigned long long* offs = nullptr;
  size_t offs_cap = 0;
  int n = -1;   // streams of the last call; -1: none to fetch
  // st_jpeg_encode_fetch: page-locked staging for the one copy of the packed streams
  uint8_t* pin = nullptr;
  size_t pin_cap = 0;
  std::vector<unsigned long long> offs_host;
  // optimize = 1: each frame's 4 x 256 symbol counts, kept for st_jpeg_encode_fetch_stats
  unsigned long long* stats = nullptr;
  size_t stats_cap = 0;
  int stats_n = -1;   // frames of the last call with optimised tables; -1: none
};

void st_jpeg_enc_release(st_ctx* ctx) {
  st_jpeg_enc_state* s = ctx->jpeg_enc;
  if (!s) return;
  if (s->params) (void)hipFree(s->params);
  if (s->blob) (void)hipFree(s->blob);
  if (s->offs) (void)hipFree(s->offs);
  if (s->stats) (void)hipFree(s->stats);
  if (s->pin) (void)hipHostFree(s->pin);
  delete s;
  ctx->jpeg_enc = nullptr;
}

namespace {

typedef unsigned long long u64;

constexpr size_t kParamsHuff = 640;   // the header's 629 bytes, padded
constexpr size_t kParamsBytes = kParamsHuff + sizeof(uint32_t) * kJpegEncHuffWords;

// ---- colour, downsampling, forward DCT, quantisation ---------------------------------------------------------------------
struct EncTransformK {
  const uint8_t* const* frames;
  int16_t* coef;          // 64 per block; blocks of an interval in MCU order, intervals frame after frame
  long long total;        // blocks in all
  int h, w, mcols, mrows;
  int nbx, nby;           // real luma blocks per row / column
  int ch;                 // chroma rows
  unsigned short div[2][64];   // 8 * the quantisation tables (luma, chroma), natural order
};

// jccolor.c in 16 fractional bits
__device__ __forceinline__ int ycc_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ __forceinline__ int ycc_c(int r, int g, int b, int c) {
  return c == 0 ? (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
                : (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// One pass of jfdctint's 8-point forward DCT (CONST_BITS 13, PASS1_BITS 2) over d[0 .. 7 * S] in place.  FIRST: outputs 0 and 4
// are << 2 and the others descaled by 11 bits; otherwise outputs 0 and 4 are descaled by 2 bits and the others by 15.
template <bool FIRST, int S>
__device__ __forceinline__ void fdct_pass(int* d) {
  const int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S], t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
  const int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S], t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int N = FIRST ? 11 : 15, R = 1 << (N - 1);
  if (FIRST) {
    d[0] = (t10 + t11) << 2;
    d[4 * S] = (t10 - t11) << 2;
  } else {
    d[0] = (t10 + t11 + 2) >> 2;
    d[4 * S] = (t10 - t11 + 2) >> 2;
  }
  int z1 = (t12 + t13) * 4433;
  d[2 * S] = (z1 + t13 * 6270 + R) >> N;
  d[6 * S] = (z1 - t12 * 15137 + R) >> N;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
  d[7 * S] = (a4 + z1 + z3 + R) >> N;
  d[5 * S] = (a5 + z2 + z4 + R) >> N;
  d[3 * S] = (a6 + z2 + z3 + R) >> N;
  d[S] = (a7 + z1 + z4 + R) >> N;
}

__device__ constexpr unsigned char kZigzag[64] = {ST_JPEG_ENC_ZIGZAG};

// Threads of an interval are numbered block-in-MCU first (all MCUs' first luma block, then their second, ...), so a wave works
// on one component and on neighbouring pixels; the block is stored at its place in MCU order.
template <int HS, int VS>
__global__ __launch_bounds__(256) void k_jpeg_fdct(EncTransformK a) {
  constexpr int NL = HS * VS, BPM = NL + 2;
  const int nblk = a.mcols * BPM;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < a.total; g += (long long)gridDim.x * 256) {
    const long long iv = g / nblk;
    const int t = (int)(g - iv * nblk);
    const int f = (int)(iv / a.mrows), my = (int)(iv - (long long)f * a.mrows);
    const int k = t / a.mcols, mx = t - k * a.mcols;
    const uint8_t* __restrict__ F = st_gl(a.frames[f]);
    const size_t pitch = (size_t)a.w * 3;
    int v[64];
    bool pad = false;
    if (k < NL) {
      int bx = mx * HS + k % HS, by = my * VS + k / HS;
      // A padding block repeats the quantised DC of the block before it in MCU order and has no AC terms: in a dummy block row
      // that is the last block of the row above in the same MCU, to the right of the picture the row's last real block.
      if (by >= a.nby) {
        pad = true;
        by = a.nby - 1;
        bx = mx * HS + HS - 1;
      }
      if (bx >= a.nbx) {
        pad = true;
        bx = a.nbx - 1;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int y = by * 8 + j < a.h ? by * 8 + j : a.h - 1;
        const uint8_t* __restrict__ R = F + (size_t)y * pitch;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int x = bx * 8 + i < a.w ? bx * 8 + i : a.w - 1;
          v[j * 8 + i] = ycc_y(R[3 * x], R[3 * x + 1], R[3 * x + 2]) - 128;
        }
      }
    } else {
      const int c = k - NL;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // the downsampled component's last row is replicated downwards; below the picture the input's last row is
        const int cy = my * 8 + j < a.ch ? my * 8 + j : a.ch - 1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int cx = mx * 8 + i;
          int acc = 0;
#pragma unroll
          for (int dy = 0; dy < VS; ++dy) {
            const int y = cy * VS + dy < a.h ? cy * VS + dy : a.h - 1;
            const uint8_t* __restrict__ R = F + (size_t)y * pitch;
#pragma unroll
            for (int dx = 0; dx < HS; ++dx) {
              const int x = cx * HS + dx < a.w ? cx * HS + dx : a.w - 1;
              acc += ycc_c(R[3 * x], R[3 * x + 1], R[3 * x + 2], c);
            }
          }
          if (HS == 2 && VS == 1) acc = (acc + (cx & 1)) >> 1;
          if (HS == 2 && VS == 2) acc = (acc + 1 + (cx & 1)) >> 2;
          v[j * 8 + i] = acc - 128;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) fdct_pass<true, 1>(v + 8 * j);
#pragma unroll
    for (int i = 0; i < 8; ++i) fdct_pass<false, 8>(v + i);
    const int tq = k < NL ? 0 : 1;
    int q[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      const unsigned d = a.div[tq][i];
      const int x = v[i];
      unsigned m = ((unsigned)(x < 0 ? -x : x) + (d >> 1)) / d;
      if (i > 0 && m > 1023u) m = 1023u;   // ten magnitude bits: no 8-bit picture gets there (st_jpeg_enc_host.h)
      q[i] = x < 0 ? -(int)m : (int)m;
      if (i > 0 && pad) q[i] = 0;
    }
    uint4* __restrict__ out = reinterpret_cast<uint4*>(a.coef + ((size_t)iv * nblk + (size_t)mx * BPM + k) * 64);
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      unsigned wd[4];
#pragma unroll
      for (int p = 0; p < 4; ++p)
        wd[p] = ((unsigned)q[kZigzag[8 * s + 2 * p]] & 0xffffu) | ((unsigned)q[kZigzag[8 * s + 2 * p + 1]] << 16);
      out[s] = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    }
  }
}

// ---- entropy coding -------------------------------------------------------------------------------------------------------
constexpr int kChunk = 64;                                                     // blocks per pass of the wave, one per lane
// OPT: the frame's own tables, whose codes may all have 16 bits: 1665 bits per block instead of 1660
template <bool OPT>
struct EncBuf {
  static constexpr int kRawBits = kChunk * (OPT ? kJpegEncBlockBitsOpt : kJpegEncBlockBits) + 7 + 7;   // carried-in bits in front, padding behind
  static constexpr int kRawWords = (kRawBits + 31) / 32 + 1;
  static constexpr int kOutBytes = ((kRawBits + 7) / 8) * 2;                   // every byte stuffed
};
constexpr int kCoefPitch = 33;                                                 // dwords per lane: 32 of coefficients + 1 against bank conflicts

struct EncEntropyK {
  const int16_t* coef;
  const uint32_t* huff;   // OPT: kJpegEncHuffWords per frame
  uint8_t* slots;
  unsigned* ilen;
  size_t slot_bytes;
  int nblk, bpm, nluma;
  int mrows;   // MCU rows per frame
};

// nb bits (the low ones of val) at bit p of the stream; bit 0 of the stream is the top bit of raw[0]
__device__ __forceinline__ void put_bits(uint32_t* raw, int p, uint32_t val, int nb) {
  const int wd = p >> 5, sh = 32 - (p & 31) - nb;
  if (sh >= 0) {
    atomicOr(&raw[wd], val << sh);
  } else {
    atomicOr(&raw[wd], val >> -sh);
    atomicOr(&raw[wd + 1], val << (32 + sh));
  }
}

// A value's magnitude category and its bits (negative values as ones' complement)
__device__ __forceinline__ void magnitude(int v, int most, int* nb, uint32_t* bits) {
  const int t = v < 0 ? -v : v;
  int n = 32 - __clz(t);   // 0 for 0
  n = n > most ? most : n;
  *nb = n;
  *bits = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
}

// jchuff's encode_one_block: the code length of the block; EMIT: also written at bit `pos`
template <bool EMIT>
__device__ __forceinline__ int code_block(const uint32_t* mine, const uint32_t* dc_tab, const uint32_t* ac_tab, int diff, uint32_t* raw, int pos) {
  int len = 0, nb;
  uint32_t mb;
  magnitude(diff, 11, &nb, &mb);
  {
    const uint32_t hc = dc_tab[nb];
    const int cl = (int)(hc >> 16);
    if (EMIT) put_bits(raw, pos, ((hc & 0xffffu) << nb) | mb, cl + nb);
    len += cl + nb;
  }
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const uint32_t wd = mine[k >> 1];
    const int v = (int)(short)((k & 1) ? (wd >> 16) : (wd & 0xffffu));
    if (v == 0) {
      ++run;
      continue;
    }
    while (run >= 16) {
      const uint32_t hc = ac_tab[0xF0];
      if (EMIT) put_bits(raw, pos + len, hc & 0xffffu, (int)(hc >> 16));
      len += (int)(hc >> 16);
      run -= 16;
    }
    magnitude(v, 10, &nb, &mb);
    const uint32_t hc = ac_tab[(run << 4) | nb];
    const int cl = (int)(hc >> 16);
    if (EMIT) put_bits(raw, pos + len, ((hc & 0xffffu) << nb) | mb, cl + nb);
    len += cl + nb;
    run = 0;
  }
  if (run > 0) {
    const uint32_t hc = ac_tab[0];
    if (EMIT) put_bits(raw, pos + len, hc & 0xffffu, (int)(hc >> 16));
    len += (int)(hc >> 16);
  }
  return len;
}

__device__ __forceinline__ int wave_inclusive_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int t = __shfl_up(v, d);
    if (lane >= d) v += t;
  }
  return v;
}

__device__ __forceinline__ unsigned raw_byte(const uint32_t* raw, int j) { return (raw[j >> 2] >> (24 - 8 * (j & 3))) & 0xffu; }

// One wave per restart interval (RESTART) or, for a stream without restart markers, per MCU row: then the row's first blocks
// take their DC predecessors from the last MCU of the row above in the same frame -- the coefficient buffer holds it, rows of a
// frame one after the other, so no workgroup depends on another --, nothing is padded with 1-bits or stuffed, the bits go to the
// slot with a zero-filled last byte, and ilen receives the row's length in BITS (at most 49 152 blocks x 1660 bits < 2^32).
// OPT: the code words are the frame's own (k_jpeg_opt_tables), any code may have 16 bits, and the buffers hold 1665 bits per block.
template <bool RESTART, bool OPT = false>
__global__ __launch_bounds__(64) void k_jpeg_entropy(EncEntropyK a) {
  constexpr int kRawWords = EncBuf<OPT>::kRawWords, kOutBytes = EncBuf<OPT>::kOutBytes;
  __shared__ uint32_t s_huff[kJpegEncHuffWords];
  __shared__ uint32_t s_coef[kChunk * kCoefPitch];
  __shared__ uint32_t s_raw[kRawWords];
  __shared__ uint8_t s_out[kOutBytes];
  const int lane = threadIdx.x;
  const size_t iv = blockIdx.x;
  const uint32_t* __restrict__ huff = OPT ? a.huff + (iv / (size_t)a.mrows) * kJpegEncHuffWords : a.huff;   // the frame's table, or the call's
  for (int i = lane; i < kJpegEncHuffWords; i += 64) s_huff[i] = huff[i];
  const int16_t* __restrict__ C = a.coef + iv * (size_t)a.nblk * 64;
  uint8_t* __restrict__ slot = a.slots + iv * a.slot_bytes;
  uint32_t* mine = s_coef + lane * kCoefPitch;
  size_t out_pos = 0;
  unsigned row_bits = 0;     // RESTART false: the row's code bits so far
  const int floor_blk = !RESTART && iv % (size_t)a.mrows != 0 ? -a.bpm : 0;   // the first block index a predecessor may have
  int carry_bits = 0;        // bits of the last, unfinished byte of the previous chunk
  uint32_t carry_val = 0;
  for (int b0 = 0; b0 < a.nblk; b0 += kChunk) {
    const int b = b0 + lane;
    const bool live = b < a.nblk;
    for (int i = lane; i < kRawWords; i += 64) s_raw[i] = 0;
    int diff = 0;
    const uint32_t *dc_tab = s_huff, *ac_tab = s_huff + 32;
    if (live) {
      const uint4* __restrict__ src = reinterpret_cast<const uint4*>(C + (size_t)b * 64);
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const uint4 t = src[s];
        mine[4 * s] = t.x; mine[4 * s + 1] = t.y; mine[4 * s + 2] = t.z; mine[4 * s + 3] = t.w;
      }
      // the DC difference to the previous block of the same component; 0 predicts the interval's first
      const int k = b % a.bpm;
      int prev;
      if (k < a.nluma) {
        prev = k > 0 ? b - 1 : b - a.bpm + a.nluma - 1;
      } else {
        prev = b - a.bpm;
        dc_tab = s_huff + 16;
        ac_tab = s_huff + 288;
      }
      // a negative index is a block of the row above (its last MCU), read only where that row belongs to this frame
      diff = (int)C[(size_t)b * 64] - (prev >= floor_blk ? (int)C[(ptrdiff_t)prev * 64] : 0);
    }
    __syncthreads();
    const int len = live ? code_block<false>(mine, dc_tab, ac_tab, diff, nullptr, 0) : 0;
    const int incl = wave_inclusive_scan(len, lane);
    int total = carry_bits + __shfl(incl, 63);
    if (lane == 0 && carry_bits) atomicOr(&s_raw[0], carry_val << (32 - carry_bits));
    if (live) (void)code_block<true>(mine, dc_tab, ac_tab, diff, s_raw, carry_bits + incl - len);
    if (!RESTART) {
      // the chunk's whole bytes as they are; after the last chunk also the unfinished byte, its low bits zero
      row_bits += (unsigned)(total - carry_bits);
      __syncthreads();
      const int nbytes = b0 + kChunk >= a.nblk ? (total + 7) >> 3 : total >> 3;
      for (int j = lane; j < nbytes; j += 64)
        if (out_pos + j < a.slot_bytes) slot[out_pos + j] = (uint8_t)raw_byte(s_raw, j);   // always: the slot holds the worst case
      out_pos += nbytes;
      carry_bits = total & 7;
      carry_val = carry_bits ? raw_byte(s_raw, total >> 3) >> (8 - carry_bits) : 0u;
      __syncthreads();
      continue;
    }
    if (b0 + kChunk >= a.nblk && (total & 7)) {   // the interval's last byte is filled with 1-bits
      const int fill = 8 - (total & 7);
      if (lane == 0) put_bits(s_raw, total, (1u << fill) - 1u, fill);
      total += fill;
    }
    __syncthreads();
    // byte stuffing: each lane takes a run of the chunk's whole bytes
    const int nbytes = total >> 3;
    const int per = (nbytes + 63) / 64;
    const int s0 = lane * per < nbytes ? lane * per : nbytes, s1 = s0 + per < nbytes ? s0 + per : nbytes;
    int ff = 0;
    for (int j = s0; j < s1; ++j) ff += raw_byte(s_raw, j) == 0xffu;
    const int ffi = wave_inclusive_scan(ff, lane);
    const int stuffed = nbytes + __shfl(ffi, 63);
    int o = s0 + ffi - ff;
    for (int j = s0; j < s1; ++j) {
      const unsigned v = raw_byte(s_raw, j);
      s_out[o++] = (uint8_t)v;
      if (v == 0xffu) s_out[o++] = 0;
    }
    carry_bits = total & 7;
    carry_val = carry_bits ? raw_byte(s_raw, nbytes) >> (8 - carry_bits) : 0u;
    __syncthreads();
    for (int j = lane; j < stuffed; j += 64)
      if (out_pos + j < a.slot_bytes) slot[out_pos + j] = s_out[j];   // always: the slot holds the worst case
    out_pos += stuffed;
    __syncthreads();
  }
  if (lane == 0) a.ilen[iv] = RESTART ? (unsigned)out_pos : row_bits;
}

// ---- layout and packing -----------------------------------------------------------------------------------------------------
struct EncLayoutK {
  const unsigned* ilen;
  u64* ioff;    // per interval: its offset in its stream
  u64* offs;    // n + 1: each stream's offset in the packed buffer, then the total
  const unsigned* hlen;   // OPT: each frame's header bytes
  int n, mrows;
};

// RESTART false: ilen holds the stuffed bytes each MCU row owns (k_jpeg_ff_count); nothing stands between them, EOI ends the stream
template <bool RESTART, bool OPT = false>
__global__ __launch_bounds__(1024) void k_jpeg_layout(EncLayoutK a) {
  __shared__ u64 part[1024];
  const int tid = threadIdx.x;
  const long long per = ((long long)a.n + 1023) / 1024;
  const long long f0 = tid * per < a.n ? tid * per : a.n, f1 = f0 + per < a.n ? f0 + per : a.n;
  u64 sum = 0;
  for (long long f = f0; f < f1; ++f) {
    u64 o = OPT ? (u64)a.hlen[f] : RESTART ? kJpegEncHeaderBytes : kJpegEncHeaderBytesNoRst;
    for (int r = 0; r < a.mrows; ++r) {
      const size_t iv = (size_t)f * a.mrows + r;
      a.ioff[iv] = o;
      o += (u64)a.ilen[iv] + (RESTART ? 2 : 0);   // the interval, then RSTn or (after the last) EOI
    }
    if (!RESTART) o += 2;
    a.offs[f] = o;   // the stream's size for now
    sum += o;
  }
  part[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    u64 run = 0;
    for (int i = 0; i < 1024; ++i) {
      const u64 p = part[i];
      part[i] = run;
      run += p;
    }
    a.offs[a.n] = run;
  }
  __syncthreads();
  u64 run = part[tid];
  for (long long f = f0; f < f1; ++f) {
    const u64 size = a.offs[f];
    a.offs[f] = run;
    run += size;
  }
}

struct EncPackK {
  const uint8_t* slots;
  const unsigned* ilen;
  const u64* ioff;
  const u64* offs;
  const uint8_t* header;   // OPT: kJpegEncHeaderStride bytes per frame, hlen[f] of them written
  const unsigned* hlen;
  uint8_t* blob;
  size_t slot_bytes;
  int mrows;
};

template <bool OPT = false>
__global__ __launch_bounds__(256) void k_jpeg_pack(EncPackK a) {
  const size_t iv = blockIdx.x;
  const size_t f = iv / (size_t)a.mrows;
  const int r = (int)(iv - f * (size_t)a.mrows);
  uint8_t* __restrict__ dst = a.blob + a.offs[f];
  if (r == 0) {
    const uint8_t* __restrict__ hd = OPT ? a.header + f * kJpegEncHeaderStride : a.header;
    const int hb = OPT ? (int)a.hlen[f] : (int)kJpegEncHeaderBytes;
    for (int j = threadIdx.x; j < hb; j += 256) dst[j] = hd[j];
  }
  const uint8_t* __restrict__ src = a.slots + iv * a.slot_bytes;
  const unsigned len = a.ilen[iv];
  uint8_t* __restrict__ d = dst + a.ioff[iv];
  for (unsigned j = threadIdx.x; j < len; j += 256) d[j] = src[j];
  if (threadIdx.x == 0) {
    d[len] = 0xFF;
    d[len + 1] = (uint8_t)(r == a.mrows - 1 ? 0xD9 : 0xD0 + (r & 7));
  }
}

// ---- streams without restart markers: the MCU rows joined bit by bit ---------------------------------------------------------
// A frame's scan before stuffing is its rows' bits one after the other, padded with 1-bits to a whole byte.  Row r starts at
// bit B(r) = the sum of the lengths above it and OWNS the bytes whose first bit lies in it: bytes ceil(B / 8) up to, not
// including, ceil((B + L) / 8).  An owned byte is 8 bits of the row's slot from bit 8 * j + sh on (sh = -B mod 8: the row's
// first sh bits completed the byte the row above owns); the last one may reach past the row's end and is completed with the
// leading bits of the next row's slot, or with 1-bits in the frame's last row.  ONE next row is enough: a row has at least 14
// bits (three blocks at least, each a DC code of 2 bits or more and an EOB of 2 (chroma) or 4 (luma)), the missing bits are
// at most 7.  So every byte of the scan has exactly one owner, which computes it from memory the entropy launch finished
// writing: no workgroup waits for another, nothing is ORed into shared bytes, nothing is read that this call did not write.
struct EncMergeK {
  const uint8_t* slots;   // per row: its bits, the last byte zero-filled (k_jpeg_entropy<false>)
  const unsigned* bits;   // per row: its length in bits
  u64* bitoff;            // per row: B, written by k_jpeg_ff_count and read by k_jpeg_pack_bits
  unsigned* slen;         // per row: the bytes it owns, stuffed zeros included
  const u64* ioff;
  const u64* offs;
  const uint8_t* header;   // OPT: kJpegEncHeaderStride bytes per frame, hlen[f] of them written
  const unsigned* hlen;
  uint8_t* blob;
  size_t slot_bytes, blob_bytes;
  int mrows;
};

// With a frame's own tables (OPT) a block may have as few as 2 bits -- a DC code of 1 bit or more and an EOB of 1 bit or more,
// or an AC symbol and its magnitude bit -- so a row has at least 6 bits at 4:4:4, 8 at 4:2:2, 12 at 4:2:0, and "one next row is
// enough" no longer holds: a byte can hold bits of three rows, a row can lie inside a byte an earlier row owns and own NO byte
// (count == 0), and the frame's padding can fall into a byte that a row before the last owns.  The ownership rule itself does
// not depend on the lengths: every byte of the scan starts in exactly one row (the rows tile the scan's bits, and the byte whose
// first bit is past the last row does not exist), that row is its one writer, and of a row's owned bytes only the last can reach
// past the row's end (the byte before it ends where the last begins, inside the row), by at most 7 bits.  Those bits are what
// FOLLOWS the row in the frame's scan: the leading bits of the next rows, as many rows as it takes -- two suffice, 6 + 6 >= 7,
// but the loop below asks only that a row has at least 1 bit and ends at the frame's last row at the latest --, then the 1-bits
// of the padding.  Each next row's contribution is read from its slot's first byte, whose bits past the row's end are zeros.
// All of it is the entropy launch's finished output, so still no workgroup waits for another.
__device__ __forceinline__ unsigned following_bits(const EncMergeK& a, size_t iv, int r) {   // the 8 bits after row r, first bit on top
  unsigned tail = 0;
  int got = 0;
  for (int rr = r + 1; rr < a.mrows && got < 8; ++rr) {
    ++iv;
    const unsigned L = a.bits[iv];
    int take = 8 - got;
    take = (unsigned)take > L ? (int)L : take;
    if (take > 0) tail |= (((unsigned)a.slots[iv * a.slot_bytes] >> (8 - take)) << (8 - got - take)) & 0xffu;
    got += take;
  }
  if (got < 8) tail |= (1u << (8 - got)) - 1u;   // past the frame's last row: the padding
  return tail;
}

struct OwnedBytes {
  const uint8_t* slot;
  u64 bits;         // L
  unsigned nvalid;  // bytes of the slot that were written: ceil(L / 8)
  unsigned count;   // owned bytes
  unsigned sh;
  unsigned tail;    // what follows the row: the next row's first byte, or 0xFF after the frame's last; OPT: following_bits()
};

template <bool OPT>
__device__ __forceinline__ OwnedBytes owned_bytes(const EncMergeK& a, size_t iv, int r, u64 B) {
  OwnedBytes o;
  o.slot = a.slots + iv * a.slot_bytes;
  o.bits = a.bits[iv];
  o.nvalid = (unsigned)((o.bits + 7) >> 3);
  const u64 first = (B + 7) >> 3;
  o.count = (unsigned)(((B + o.bits + 7) >> 3) - first);
  o.sh = (unsigned)(first * 8 - B);
  if (OPT) o.tail = following_bits(a, iv, r);
  else o.tail = r == a.mrows - 1 ? 0xffu : a.slots[(iv + 1) * a.slot_bytes];
  return o;
}

__device__ __forceinline__ unsigned owned_byte(const OwnedBytes& o, unsigned j) {   // j < o.count, hence j < o.nvalid
  unsigned v = o.slot[j];
  if (o.sh) v = ((v << o.sh) | (j + 1 < o.nvalid ? (unsigned)o.slot[j + 1] >> (8 - o.sh) : 0u)) & 0xffu;
  const u64 end = (u64)j * 8 + o.sh + 8;   // past the row's end by 1 .. 7 bits, which the slot holds as zeros
  if (end > o.bits) v |= o.tail >> (8 - (unsigned)(end - o.bits));
  return v;
}

__device__ __forceinline__ u64 block_sum(u64 v, u64* red) {   // 256 threads
  red[threadIdx.x] = v;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
    __syncthreads();
  }
  v = red[0];
  __syncthreads();
  return v;
}

// One workgroup per MCU row: its bit offset in the frame's scan (the lengths above it summed; at most 8192 rows) and the
// number of bytes it owns, a zero after every 0xFF among them counted in.
template <bool OPT = false>
__global__ __launch_bounds__(256) void k_jpeg_ff_count(EncMergeK a) {
  __shared__ u64 red[256];
  const size_t iv = blockIdx.x;
  const size_t f = iv / (size_t)a.mrows;
  const int r = (int)(iv - f * (size_t)a.mrows);
  u64 part = 0;
  for (int i = threadIdx.x; i < r; i += 256) part += a.bits[f * (size_t)a.mrows + i];
  const u64 B = block_sum(part, red);
  const OwnedBytes o = owned_bytes<OPT>(a, iv, r, B);
  u64 ff = 0;
  for (unsigned j = threadIdx.x; j < o.count; j += 256) ff += owned_byte(o, j) == 0xffu;
  ff = block_sum(ff, red);
  if (threadIdx.x == 0) {
    a.bitoff[iv] = B;
    a.slen[iv] = o.count + (unsigned)ff;
  }
}

// One workgroup per MCU row: the header (the frame's first row), the row's owned bytes with their stuffed zeros -- computed
// again, 256 at a time, a ballot and a prefix over the four waves placing them --, EOI after the frame's last row.
template <bool OPT = false>
__global__ __launch_bounds__(256) void k_jpeg_pack_bits(EncMergeK a) {
  __shared__ unsigned s_w[4];
  const size_t iv = blockIdx.x;
  const size_t f = iv / (size_t)a.mrows;
  const int r = (int)(iv - f * (size_t)a.mrows);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u64 at = a.offs[f];
  const u64 room = at < a.blob_bytes ? a.blob_bytes - at : 0;   // every store below stays inside the blob
  uint8_t* __restrict__ dst = a.blob + at;
  if (r == 0) {
    const uint8_t* __restrict__ hd = OPT ? a.header + f * kJpegEncHeaderStride : a.header;
    const int hb = OPT ? (int)a.hlen[f] : (int)kJpegEncHeaderBytesNoRst;
    for (int j = tid; j < hb; j += 256)
      if ((u64)j < room) dst[j] = hd[j];
  }
  const OwnedBytes o = owned_bytes<OPT>(a, iv, r, a.bitoff[iv]);
  const u64 base = a.ioff[iv];
  unsigned ff_run = 0;
  for (unsigned t0 = 0; t0 < o.count; t0 += 256) {
    const unsigned j = t0 + tid;
    const bool live = j < o.count;
    const unsigned v = live ? owned_byte(o, j) : 0u;
    const bool ff = v == 0xffu;
    const u64 m = __ballot(ff);
    if (lane == 0) s_w[wave] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned before = (unsigned)__popcll(m & ((1ull << lane) - 1ull)), all = 0;
    for (int k = 0; k < 4; ++k) {
      before += k < wave ? s_w[k] : 0u;
      all += s_w[k];
    }
    const u64 pos = base + j + ff_run + before;
    if (live && pos < room) dst[pos] = (uint8_t)v;
    if (ff && pos + 1 < room) dst[pos + 1] = 0;
    ff_run += all;
    __syncthreads();
  }
  if (r == a.mrows - 1 && tid == 0) {
    const u64 pos = base + o.count + ff_run;
    if (pos + 1 < room) {
      dst[pos] = 0xFF;
      dst[pos + 1] = 0xD9;
    }
  }
}

// ---- optimised Huffman tables: each frame's symbol counts and the tables built from them ---------------------
struct EncStatsK {
  const int16_t* coef;
  u64* freq;   // per frame kJpegOptTables x 256 counters, zeroed by the call before this launch
  int nblk, bpm, nluma, mrows;
};

// One wave per MCU row, the work unit and block numbering of k_jpeg_entropy: each lane walks its block once and counts the
// symbols code_block would emit (st_jpeg_opt_block_symbols) in the workgroup's 4 x 256 LDS counters -- 32 bits are plenty for a
// row: at most 49 152 blocks of 64 symbols --, which are then added to the frame's 64-bit counters.  Integer adds: the sums do
// not depend on the order.  RESTART false: the row's first blocks take their DC predecessor from the row above.
template <bool RESTART>
__global__ __launch_bounds__(64) void k_jpeg_sym_stats(EncStatsK a) {
  __shared__ uint32_t s_coef[kChunk * kCoefPitch];
  __shared__ unsigned s_hist[kJpegOptTables * 256];
  const int lane = threadIdx.x;
  const size_t iv = blockIdx.x;
  for (int i = lane; i < kJpegOptTables * 256; i += 64) s_hist[i] = 0;
  const int16_t* __restrict__ C = a.coef + iv * (size_t)a.nblk * 64;
  uint32_t* mine = s_coef + lane * kCoefPitch;
  const int floor_blk = !RESTART && iv % (size_t)a.mrows != 0 ? -a.bpm : 0;
  __syncthreads();
  for (int b0 = 0; b0 < a.nblk; b0 += kChunk) {
    const int b = b0 + lane;
    if (b < a.nblk) {
      const uint4* __restrict__ src = reinterpret_cast<const uint4*>(C + (size_t)b * 64);
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const uint4 t = src[s];
        mine[4 * s] = t.x; mine[4 * s + 1] = t.y; mine[4 * s + 2] = t.z; mine[4 * s + 3] = t.w;
      }
      const int k = b % a.bpm;
      const bool luma = k < a.nluma;
      const int prev = luma ? (k > 0 ? b - 1 : b - a.bpm + a.nluma - 1) : b - a.bpm;
      const int diff = (int)C[(size_t)b * 64] - (prev >= floor_blk ? (int)C[(ptrdiff_t)prev * 64] : 0);
      unsigned* hist = s_hist + (luma ? 0 : 2 * 256);   // the component's DC table; its AC table follows
      st_jpeg_opt_block_symbols(
          [mine](int p) {
            const uint32_t wd = mine[p >> 1];
            return (int)(short)((p & 1) ? (wd >> 16) : (wd & 0xffffu));
          },
          diff, [hist](int ac, int sym) { atomicAdd(&hist[ac * 256 + (sym & 255)], 1u); });
    }
  }
  __syncthreads();
  u64* __restrict__ F = a.freq + (iv / (size_t)a.mrows) * (size_t)(kJpegOptTables * 256);
  for (int i = lane; i < kJpegOptTables * 256; i += 64) {
    const unsigned c = s_hist[i];
    if (c) atomicAdd(&F[i], (u64)c);
  }
}

struct EncTablesK {
  const u64* freq;
  const uint8_t* fixed;   // the call's header with the Annex K tables: its prefix and what follows its DHT segments are copied
  uint32_t* huff;         // per frame kJpegEncHuffWords code words
  uint8_t* headers;       // per frame kJpegEncHeaderStride bytes
  unsigned* hlen;         // per frame: the header's bytes
  unsigned fixed_bytes;   // 623 or 629
};

__device__ __forceinline__ void wave_least(const uint64_t* freq, int lane, int exclude, int* idx) {
  // 257 entries over 64 lanes, 5 each (the last lanes none); then a butterfly whose every step keeps the better candidate --
  // the rule is a total order on (frequency, index), so all lanes end on the serial search's choice, ties included
  const int lo = lane * 5 < kJpegOptSymbols ? lane * 5 : kJpegOptSymbols, hi = lo + 5 < kJpegOptSymbols ? lo + 5 : kJpegOptSymbols;
  uint64_t v;
  int i = st_jpeg_opt_least(freq, lo, hi, exclude, &v);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint64_t ov = (uint64_t)__shfl_xor((u64)v, d);
    const int oi = __shfl_xor(i, d);
    if (!st_jpeg_opt_better(v, i, ov, oi)) {
      v = ov;
      i = oi;
    }
  }
  *idx = i;
}

// One workgroup per frame, one wave per table (DC luma, AC luma, DC chroma, AC chroma): the merge loop of
// jpeg_gen_optimal_table is serial -- at most 256 steps --, the wave shares each step's two searches for the least frequency
// and lane 0 merges.  The steps are separated by workgroup barriers (the four waves take the same number of trips: until none
// has two entries left), so nothing relies on the order of LDS accesses inside a wave.  When all four tables are known, their
// lengths are, and each wave writes its code words and its DHT segment at its place in the frame's header: SOI .. SOF0 from the
// call's header, DHT x 4, then DRI (MCU_ROW only) and SOS from the call's header.
__global__ __launch_bounds__(256) void k_jpeg_opt_tables(EncTablesK a) {
  __shared__ StJpegOptWork s_w[kJpegOptTables];
  __shared__ uint8_t s_bits[kJpegOptTables][16];
  __shared__ uint8_t s_vals[kJpegOptTables][256];
  __shared__ int s_nvals[kJpegOptTables];
  const size_t f = blockIdx.x;
  const int lane = threadIdx.x & 63, t = threadIdx.x >> 6;
  StJpegOptWork* w = &s_w[t];
  for (int i = lane; i < kJpegOptSymbols; i += 64) st_jpeg_opt_begin(w, i, i < 256 ? a.freq[f * (size_t)(kJpegOptTables * 256) + t * 256 + i] : 1);
  __syncthreads();
  for (int step = 0; step < kJpegOptSymbols; ++step) {
    int c1, c2;
    wave_least(w->freq, lane, -1, &c1);
    wave_least(w->freq, lane, c1, &c2);
    if (!__syncthreads_or(c2 >= 0)) break;   // every search has read before any merge writes; no table has two entries left
    if (lane == 0 && c2 >= 0) st_jpeg_opt_merge(w->freq, w->codesize, w->others, c1, c2);
    __syncthreads();
  }
  if (lane == 0) {
    int nv = 0;
    (void)st_jpeg_opt_lengths(w->codesize, s_bits[t], s_vals[t], &nv);
    s_nvals[t] = nv;
    st_jpeg_opt_codes(s_bits[t], s_vals[t], nv, a.huff + f * kJpegEncHuffWords + st_jpeg_opt_tab_off(t), st_jpeg_opt_tab_words(t));
  }
  __syncthreads();
  unsigned off = (unsigned)kJpegEncHeaderPrefix;
  for (int u = 0; u < t; ++u) off += (unsigned)st_jpeg_opt_dht_bytes(s_nvals[u]);
  const unsigned mine = (unsigned)st_jpeg_opt_dht_bytes(s_nvals[t]);
  uint8_t* __restrict__ H = a.headers + f * kJpegEncHeaderStride;
  // at most 12 DC and 162 AC symbols are ever counted, so off + mine + 20 <= 629; the checks keep the stores inside whatever
  for (unsigned i = lane; i < mine; i += 64)
    if (off + i < kJpegEncHeaderStride) H[off + i] = st_jpeg_opt_dht_byte(s_bits[t], s_vals[t], s_nvals[t], st_jpeg_opt_class_id(t), (int)i);
  if (t == 0)
    for (unsigned i = lane; i < kJpegEncHeaderPrefix; i += 64) H[i] = a.fixed[i];
  if (t == kJpegOptTables - 1) {
    const unsigned end = off + mine, from = (unsigned)kJpegEncHeaderBytesNoRst - 14u;   // where DRI or SOS begins in the call's header
    const unsigned rest = a.fixed_bytes - from;
    for (unsigned i = lane; i < rest; i += 64)
      if (end + i < kJpegEncHeaderStride) H[end + i] = a.fixed[from + i];
    if (lane == 0) a.hlen[f] = end + rest < kJpegEncHeaderStride ? end + rest : (unsigned)kJpegEncHeaderStride;
  }
}

template <class T>
int grow(st_ctx* ctx, T** p, size_t* cap, size_t want, const char* what) {
  if (want <= *cap) return ST_OK;
  if (*p) ST_HIP(ctx, hipFree(*p));   // waits for the device
  *p = nullptr;
  *cap = 0;
  const size_t bytes = (want + want / 4) * sizeof(T);
  const hipError_t e = hipMalloc((void**)p, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    return st_set_error(ctx, ST_ERR_OOM, "jpeg_encode: hipMalloc(%zu) for %s failed: %s", bytes, what, hipGetErrorString(e));
  }
  *cap = want + want / 4;
  return ST_OK;
}

// optimize = 0 is st_jpeg_encode_batch_rst as it always was: every `opt` below only adds to it
int encode_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int quality, int h_samp, int v_samp, int restart, int optimize) {
  ST_TRY(st_enter(ctx));
  if (!ctx->jpeg_enc) ctx->jpeg_enc = new st_jpeg_enc_state();
  st_jpeg_enc_state* s = ctx->jpeg_enc;
  s->n = -1;   // a call that fails leaves nothing to fetch
  s->stats_n = -1;
  char msg[160];
  if (st_jpeg_enc_check_restart(restart, msg, sizeof msg) != ST_OK) return st_set_error(ctx, ST_ERR_INVALID, "jpeg_encode: %s", msg);
  if (st_jpeg_enc_check_optimize(optimize, msg, sizeof msg) != ST_OK) return st_set_error(ctx, ST_ERR_INVALID, "jpeg_encode: %s", msg);
  const bool rst = restart == ST_JPEG_RESTART_ROW, opt = optimize == 1;
  if (n < 0) return st_set_error(ctx, ST_ERR_INVALID, "jpeg_encode: n = %d is negative", n);
  const int chk = st_jpeg_enc_check(h, w, quality, h_samp, v_samp, msg, sizeof msg);
  if (chk != ST_OK) return st_set_error(ctx, chk, "jpeg_encode: %s", msg);
  if (n == 0) {
    s->n = 0;
    return ST_OK;
  }
  if (!frames_dev) return st_set_error(ctx, ST_ERR_INVALID, "jpeg_encode: null frame table");
  ST_TRY(st_check_rows(ctx, "jpeg_encode: frame %d is a null pointer", n, false, frames_dev));
  StJpegEncGeom g;
  st_jpeg_enc_geom(h, w, h_samp, v_samp, &g);
  const long long intervals = (long long)n * g.mrows;
  if (intervals > INT_MAX) return st_set_error(ctx, ST_ERR_UNSUPPORTED, "jpeg_encode: %lld restart intervals in one call (at most 2^31 - 1)", intervals);
  const int nblk = g.mcols * g.bpm;
  // without markers a slot holds the row's bits as they are, half of what they could take stuffed
  // with the frame's own tables a block has up to 1665 bits: 418 / 209 bytes per block instead of 416 / 208
  const size_t opt_slot = ((size_t)nblk * (rst ? kJpegEncBlockStuffedOpt : kJpegEncBlockBytesOpt) + 15) / 16 * 16;
  const size_t slot_bytes = opt ? opt_slot : rst ? st_jpeg_enc_slot_bytes(g) : st_jpeg_enc_raw_slot_bytes(g);
  const size_t bound = (size_t)(opt ? st_jpeg_encode_bound_opt(h, w, h_samp, v_samp) : st_jpeg_encode_bound(h, w, h_samp, v_samp));

  // header and code tables, when the call differs from the last one
  const int key[6] = {h, w, quality, h_samp, v_samp, restart};
  if (!s->params) {
    ST_HIP(ctx, hipMalloc((void**)&s->params, kParamsBytes));
    memset(s->key, 0, sizeof s->key);
  }
  if (memcmp(key, s->key, sizeof key) != 0) {
    ST_HIP(ctx, hipStreamSynchronize(ctx->stream));   // an earlier upload may still read params_host
    s->params_host.assign(kParamsBytes, 0);
    size_t hb = 0;
    (void)st_jpeg_encode_header_rst(h, w, quality, h_samp, v_samp, restart, s->params_host.data(), kParamsHuff, &hb);
    st_jpeg_enc_huff(reinterpret_cast<uint32_t*>(s->params_host.data() + kParamsHuff));
    memset(s->key, 0, sizeof s->key);
    ST_HIP(ctx, hipMemcpyAsync(s->params, s->params_host.data(), kParamsBytes, hipMemcpyHostToDevice, ctx->stream));
    memcpy(s->key, key, sizeof key);
  }
  ST_TRY(grow(ctx, &s->blob, &s->blob_cap, (size_t)n * bound, "the streams"));
  ST_TRY(grow(ctx, &s->offs, &s->offs_cap, (size_t)n + 1, "the stream offsets"));
  if (opt) ST_TRY(grow(ctx, &s->stats, &s->stats_cap, (size_t)n * (kJpegOptTables * 256), "the symbol counts"));

  const size_t cb = (size_t)intervals * (size_t)nblk * 128, sb = (size_t)intervals * slot_bytes;
  const size_t lb = sizeof(unsigned) * (size_t)intervals, ob = sizeof(u64) * (size_t)intervals;
  // the frames' own code words, headers and header lengths
  const size_t hwb = sizeof(uint32_t) * kJpegEncHuffWords * (size_t)n, hdb = kJpegEncHeaderStride * (size_t)n, hlb = sizeof(unsigned) * (size_t)n;
  const uint8_t** d_frames;
  ST_TRY(st_upload_tables(ctx, n, st_align_up(cb) + st_align_up(sb) + st_align_up(lb) + st_align_up(ob) + (rst ? 0 : st_align_up(lb) + st_align_up(ob)) +
                                  (opt ? st_align_up(hwb) + st_align_up(hdb) + st_align_up(hlb) : 0), frames_dev, &d_frames));
  int16_t* d_coef = (int16_t*)st_ws_alloc(ctx, cb);
  uint8_t* d_slots = (uint8_t*)st_ws_alloc(ctx, sb);
  unsigned* d_ilen = (unsigned*)st_ws_alloc(ctx, lb);
  u64* d_ioff = (u64*)st_ws_alloc(ctx, ob);
  unsigned* d_slen = rst ? d_ilen : (unsigned*)st_ws_alloc(ctx, lb);   // without markers: the rows' bits, and their stuffed bytes
  u64* d_bitoff = rst ? d_ioff : (u64*)st_ws_alloc(ctx, ob);
  uint32_t* d_huff = opt ? (uint32_t*)st_ws_alloc(ctx, hwb) : nullptr;
  uint8_t* d_headers = opt ? (uint8_t*)st_ws_alloc(ctx, hdb) : nullptr;
  unsigned* d_hlen = opt ? (unsigned*)st_ws_alloc(ctx, hlb) : nullptr;
  if (!d_coef || !d_slots || !d_ilen || !d_ioff || !d_slen || !d_bitoff || (opt && (!d_huff || !d_headers || !d_hlen)))
    return st_set_error(ctx, ST_ERR_OOM, "jpeg_encode: workspace exhausted");

  EncTransformK t;
  t.frames = d_frames; t.coef = d_coef; t.total = intervals * nblk;
  t.h = h; t.w = w; t.mcols = g.mcols; t.mrows = g.mrows; t.nbx = g.nbx; t.nby = g.nby; t.ch = g.ch;
  uint16_t q[2][64];
  (void)st_jpeg_quant_tables(quality, q[0], q[1]);
  for (int c = 0; c < 2; ++c)
    for (int i = 0; i < 64; ++i) t.div[c][i] = (unsigned short)(q[c][i] * 8);
  {
    const long long wgs = (t.total + 255) / 256;
    const dim3 grid((unsigned)(wgs < 0x7fffffffLL ? wgs : 0x7fffffffLL));
    st_timed tm(ctx, ST_K_JPEG);
    if (h_samp == 1) hipLaunchKernelGGL((k_jpeg_fdct<1, 1>), grid, dim3(256), 0, ctx->stream, t);
    else if (v_samp == 1) hipLaunchKernelGGL((k_jpeg_fdct<2, 1>), grid, dim3(256), 0, ctx->stream, t);
    else hipLaunchKernelGGL((k_jpeg_fdct<2, 2>), grid, dim3(256), 0, ctx->stream, t);
    ST_HIP(ctx, hipGetLastError());
  }
  if (opt) {
    // the counters are zeroed on the stream, in front of the launch that adds to them: nothing depends on an earlier call
    ST_HIP(ctx, hipMemsetAsync(s->stats, 0, sizeof(u64) * (size_t)n * (kJpegOptTables * 256), ctx->stream));
    EncStatsK c;
    c.coef = d_coef; c.freq = s->stats; c.nblk = nblk; c.bpm = g.bpm; c.nluma = g.bpm - 2; c.mrows = g.mrows;
    {
      st_timed tm(ctx, ST_K_JPEG);
      if (rst) hipLaunchKernelGGL(k_jpeg_sym_stats<true>, dim3((unsigned)intervals), dim3(64), 0, ctx->stream, c);
      else hipLaunchKernelGGL(k_jpeg_sym_stats<false>, dim3((unsigned)intervals), dim3(64), 0, ctx->stream, c);
      ST_HIP(ctx, hipGetLastError());
    }
    EncTablesK b;
    b.freq = s->stats; b.fixed = s->params; b.huff = d_huff; b.headers = d_headers; b.hlen = d_hlen;
    b.fixed_bytes = (unsigned)st_jpeg_enc_header_bytes(restart);
    {
      st_timed tm(ctx, ST_K_JPEG);
      hipLaunchKernelGGL(k_jpeg_opt_tables, dim3((unsigned)n), dim3(256), 0, ctx->stream, b);
      ST_HIP(ctx, hipGetLastError());
    }
  }
  EncEntropyK e;
  e.coef = d_coef; e.huff = opt ? d_huff : reinterpret_cast<const uint32_t*>(s->params + kParamsHuff); e.slots = d_slots; e.ilen = d_ilen;
  e.slot_bytes = slot_bytes; e.nblk = nblk; e.bpm = g.bpm; e.nluma = g.bpm - 2; e.mrows = g.mrows;
  {
    st_timed tm(ctx, ST_K_JPEG);
    const dim3 grid((unsigned)intervals);
    if (opt && rst) hipLaunchKernelGGL((k_jpeg_entropy<true, true>), grid, dim3(64), 0, ctx->stream, e);
    else if (opt) hipLaunchKernelGGL((k_jpeg_entropy<false, true>), grid, dim3(64), 0, ctx->stream, e);
    else if (rst) hipLaunchKernelGGL(k_jpeg_entropy<true>, grid, dim3(64), 0, ctx->stream, e);
    else hipLaunchKernelGGL(k_jpeg_entropy<false>, grid, dim3(64), 0, ctx->stream, e);
    ST_HIP(ctx, hipGetLastError());
  }
  EncMergeK m;
  m.slots = d_slots; m.bits = d_ilen; m.bitoff = d_bitoff; m.slen = d_slen; m.ioff = d_ioff; m.offs = s->offs;
  m.header = opt ? d_headers : s->params; m.hlen = d_hlen;
  m.blob = s->blob; m.slot_bytes = slot_bytes; m.blob_bytes = (size_t)n * bound; m.mrows = g.mrows;
  if (!rst) {
    st_timed tm(ctx, ST_K_JPEG);
    if (opt) hipLaunchKernelGGL(k_jpeg_ff_count<true>, dim3((unsigned)intervals), dim3(256), 0, ctx->stream, m);
    else hipLaunchKernelGGL(k_jpeg_ff_count<false>, dim3((unsigned)intervals), dim3(256), 0, ctx->stream, m);
    ST_HIP(ctx, hipGetLastError());
  }
  EncLayoutK l;
  l.ilen = d_slen; l.ioff = d_ioff; l.offs = s->offs; l.hlen = d_hlen; l.n = n; l.mrows = g.mrows;
  {
    st_timed tm(ctx, ST_K_JPEG);
    if (opt && rst) hipLaunchKernelGGL((k_jpeg_layout<true, true>), dim3(1), dim3(1024), 0, ctx->stream, l);
    else if (opt) hipLaunchKernelGGL((k_jpeg_layout<false, true>), dim3(1), dim3(1024), 0, ctx->stream, l);
    else if (rst) hipLaunchKernelGGL(k_jpeg_layout<true>, dim3(1), dim3(1024), 0, ctx->stream, l);
    else hipLaunchKernelGGL(k_jpeg_layout<false>, dim3(1), dim3(1024), 0, ctx->stream, l);
    ST_HIP(ctx, hipGetLastError());
  }
  if (!rst) {
    st_timed tm(ctx, ST_K_JPEG);
    if (opt) hipLaunchKernelGGL(k_jpeg_pack_bits<true>, dim3((unsigned)intervals), dim3(256), 0, ctx->stream, m);
    else hipLaunchKernelGGL(k_jpeg_pack_bits<false>, dim3((unsigned)intervals), dim3(256), 0, ctx->stream, m);
    ST_HIP(ctx, hipGetLastError());
    s->n = n;
    if (opt) s->stats_n = n;
    return ST_OK;
  }
  EncPackK p;
  p.slots = d_slots; p.ilen = d_ilen; p.ioff = d_ioff; p.offs = s->offs; p.header = opt ? d_headers : s->params; p.hlen = d_hlen; p.blob = s->blob;
  p.slot_bytes = slot_bytes; p.mrows = g.mrows;
  {
    st_timed tm(ctx, ST_K_JPEG);
    if (opt) hipLaunchKernelGGL(k_jpeg_pack<true>, dim3((unsigned)intervals), dim3(256), 0, ctx->stream, p);
    else hipLaunchKernelGGL(k_jpeg_pack<false>, dim3((unsigned)intervals), dim3(256), 0, ctx->stream, p);
    ST_HIP(ctx, hipGetLastError());
  }
  s->n = n;
  if (opt) s->stats_n = n;
  return ST_OK;
}

}  // namespace

ST_EXPORT int st_jpeg_encode_batch_rst(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int quality, int h_samp, int v_samp,
                                       int restart) {
  return encode_batch(ctx, frames_dev, n, h, w, quality, h_samp, v_samp, restart, 0);
}

ST_EXPORT int st_jpeg_encode_batch_opt(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int quality, int h_samp, int v_samp,
                                       int restart, int optimize) {
  return encode_batch(ctx, frames_dev, n, h, w, quality, h_samp, v_samp, restart, optimize);
}

ST_EXPORT int st_jpeg_encode_fetch_stats(st_ctx* ctx, uint64_t* freq, size_t cap) {
  ST_TRY(st_enter(ctx));
  st_jpeg_enc_state* s = ctx->jpeg_enc;
  if (!s || s->stats_n < 0) return st_set_error(ctx, ST_ERR_INVALID, "jpeg_encode_fetch_stats: no st_jpeg_encode_batch_opt call with optimize = 1 to fetch from");
  const size_t count = (size_t)s->stats_n * (kJpegOptTables * 256);
  if (!freq || cap < count) return st_set_error(ctx, ST_ERR_INVALID, "jpeg_encode_fetch_stats: %zu counters, room for %zu", count, freq ? cap : (size_t)0);
  ST_HIP(ctx, hipMemcpyAsync(freq, s->stats, sizeof(uint64_t) * count, hipMemcpyDeviceToHost, ctx->stream));
  ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ST_OK;
}

ST_EXPORT int st_jpeg_encode_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int quality, int h_samp, int v_samp) {
  return st_jpeg_encode_batch_rst(ctx, frames_dev, n, h, w, quality, h_samp, v_samp, ST_JPEG_RESTART_ROW);
}

ST_EXPORT int st_jpeg_encode_fetch(st_ctx* ctx, uint8_t* const* bufs_host, size_t* sizes, size_t capacity) {
  ST_TRY(st_enter(ctx));
  st_jpeg_enc_state* s = ctx->jpeg_enc;
  if (!s || s->n < 0) return st_set_error(ctx, ST_ERR_INVALID, "jpeg_encode_fetch: no st_jpeg_encode_batch call to fetch from");
  if (s->n == 0) return ST_OK;
  if (!sizes) return st_set_error(ctx, ST_ERR_INVALID, "jpeg_encode_fetch: null sizes");
  const size_t n = (size_t)s->n;
  s->offs_host.resize(n + 1);
  ST_HIP(ctx, hipMemcpyAsync(s->offs_host.data(), s->offs, sizeof(u64) * (n + 1), hipMemcpyDeviceToHost, ctx->stream));
  ST_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the one wait for the kernels
  size_t most = 0;
  for (size_t i = 0; i < n; ++i) {
    sizes[i] = (size_t)(s->offs_host[i + 1] - s->offs_host[i]);
    most = sizes[i] > most ? sizes[i] : most;
  }
  if (!bufs_host) return ST_OK;   // the sizes alone
  if (most > capacity) return st_set_error(ctx, ST_ERR_INVALID, "jpeg_encode_fetch: a stream has %zu bytes, the buffers hold %zu", most, capacity);
  for (size_t i = 0; i < n; ++i)
    if (!bufs_host[i]) return st_set_error(ctx, ST_ERR_INVALID, "jpeg_encode_fetch: buffer %zu is a null pointer", i);
  const size_t total = (size_t)s->offs_host[n];
  if (total > s->pin_cap) {
    if (s->pin) ST_HIP(ctx, hipHostFree(s->pin));
    s->pin = nullptr;
    s->pin_cap = 0;
    const size_t want = total + total / 4;
    if (hipHostMalloc((void**)&s->pin, want, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      s->pin = nullptr;
      return st_set_error(ctx, ST_ERR_OOM, "jpeg_encode_fetch: cannot page-lock %zu bytes for the streams", want);
    }
    s->pin_cap = want;
  }
  ST_HIP(ctx, hipMemcpyAsync(s->pin, s->blob, total, hipMemcpyDeviceToHost, ctx->stream));   // every stream in one copy
  ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n; ++i) memcpy(bufs_host[i], s->pin + s->offs_host[i], sizes[i]);
  return ST_OK;
}
