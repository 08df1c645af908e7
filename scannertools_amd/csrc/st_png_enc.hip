// ImageEncoder, PNG (opt-in): rows filtered, the filtered bytes deflated in independent pieces of 32 768, every piece one IDAT
// chunk.  DESIGN.md 4.18; the bytes are those of st_png_encode_host (st_png_enc_host.cpp), which shares st_png_enc.h.
//
// k_png_filter   one workgroup per row, sixteen bytes per thread and step (dword loads and stores at any alignment): the five
//                filters' sums of min(b, 256 - b), the type, the filtered row.
// k_png_deflate  one workgroup per piece, the piece in LDS: run boundaries per 128-byte stretch, the token of every position in
//                closed form (st_png_token), the symbol counts, the two codes (ranking, depths, lengths, canonical codes and
//                the header's offsets by all threads; the merges and the 19-symbol code by one), the tokens' bit offsets, the bits ORed into an LDS buffer, stored instead where that is not
//                shorter, then the chunk -- length, type, data, CRC-32 -- into the piece's slot, and the piece's Adler sums.
// k_png_enc_layout  one workgroup: the chunks' places in the packed streams and the n + 1 stream offsets.
// k_png_enc_pack    one workgroup per piece: its chunk into place; a frame's first adds signature and IHDR, its last the
//                closing IDAT (the Adler-32 folded from the pieces' sums) and IEND.
// No workgroup waits for another inside a launch.
#include <climits>
#include <cstring>
#include <vector>

#include "st_internal.h"
#include "st_png_enc.h"

extern "C" int st_png_enc_check(int h, int w, int c, int filter, char* msg, size_t msg_len);   // st_png_enc_host.cpp

namespace {

typedef unsigned long long u64;
typedef unsigned u32u __attribute__((aligned(1)));

constexpr int kStretch = kPngPiece / 256;   // positions a thread of k_png_deflate owns
constexpr int kCrcSeg = 129;                // bytes of a chunk's type and data a thread sums: 256 x 129 >= 4 + 2 + 5 + 32 768
constexpr int kBitWords = (kPngPiece + 8) / 4 + 6;
static_assert(256 * kCrcSeg >= 4 + 2 + 5 + kPngPiece, "the CRC segments cover the longest chunk");

struct PngFilterK {
  const uint8_t* const* frames;
  uint8_t* filt;
  size_t stride;
  long long rows;
  int h, rb, bpp, filter;
};

__device__ __forceinline__ unsigned png_ld32(const uint8_t* p) { return *reinterpret_cast<const u32u*>(p); }

// Sixteen bytes of a row at a time: i0 is a multiple of 16, the row's bytes i0 .. i0 + 15 and the four in front of them (the left
// neighbours of the first BPP) as five dwords at any alignment, the same of the row above.  f(t, x, a, b, c) for t = 0 .. 15 with
// constant indices, so everything stays in registers.  The row's last bytes, fewer than sixteen, go bytewise: nothing is read
// past the row.
template <int BPP, class F>
__device__ __forceinline__ void png_row16(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ up, bool has_up, int i0, F f) {
  unsigned x[5], u[5];
  x[0] = i0 ? png_ld32(cur + i0 - 4) : 0u;
  u[0] = has_up && i0 ? png_ld32(up + i0 - 4) : 0u;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    x[q + 1] = png_ld32(cur + i0 + 4 * q);
    u[q + 1] = has_up ? png_ld32(up + i0 + 4 * q) : 0u;
  }
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int at = 4 + t, left = at - BPP;
    f(t, (int)((x[at >> 2] >> (8 * (at & 3))) & 0xffu), (int)((x[left >> 2] >> (8 * (left & 3))) & 0xffu), (int)((u[at >> 2] >> (8 * (at & 3))) & 0xffu),
      (int)((u[left >> 2] >> (8 * (left & 3))) & 0xffu));
  }
}

template <int BPP>
__device__ __forceinline__ void png_filter_row(const PngFilterK& a, const uint8_t* __restrict__ cur, const uint8_t* __restrict__ up, bool has_up,
                                               uint8_t* __restrict__ o, unsigned (*s_sum)[5]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rb = a.rb;
  const int whole = rb & ~15;   // bytes in chunks of sixteen
  int ft = a.filter;
  if (ft == ST_PNG_FILTER_ADAPTIVE) {
    unsigned sum[5] = {0u, 0u, 0u, 0u, 0u};   // a row has at most 262 140 bytes of at most 128 each
    for (int i0 = 16 * tid; i0 < whole; i0 += 16 * 256)
      png_row16<BPP>(cur, up, has_up, i0, [&](int, int x, int av, int bv, int cv) {
#pragma unroll
        for (int t = 0; t < 5; ++t) sum[t] += st_png_filter_cost(st_png_filter_byte(t, x, av, bv, cv));
      });
    for (int i = whole + tid; i < rb; i += 256) {
      const int x = cur[i], av = i >= BPP ? cur[i - BPP] : 0, bv = has_up ? up[i] : 0, cv = has_up && i >= BPP ? up[i - BPP] : 0;
#pragma unroll
      for (int t = 0; t < 5; ++t) sum[t] += st_png_filter_cost(st_png_filter_byte(t, x, av, bv, cv));
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      unsigned v = sum[t];
      for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
      if (lane == 0) s_sum[wave][t] = v;
    }
    __syncthreads();
    unsigned best = 0xffffffffu;
    for (int t = 0; t < 5; ++t) {
      const unsigned v = s_sum[0][t] + s_sum[1][t] + s_sum[2][t] + s_sum[3][t];
      if (v < best) {   // ties stay with the lower type
        best = v;
        ft = t;
      }
    }
  }
  if (tid == 0) o[0] = (uint8_t)ft;
  for (int i0 = 16 * tid; i0 < whole; i0 += 16 * 256) {
    unsigned w[4] = {0u, 0u, 0u, 0u};
    png_row16<BPP>(cur, up, has_up, i0, [&](int t, int x, int av, int bv, int cv) { w[t >> 2] |= st_png_filter_byte(ft, x, av, bv, cv) << (8 * (t & 3)); });
#pragma unroll
    for (int q = 0; q < 4; ++q) reinterpret_cast<u32u*>(o + 1 + i0)[q] = w[q];   // the type byte puts the row at an odd offset
  }
  for (int i = whole + tid; i < rb; i += 256) {
    const int x = cur[i], av = i >= BPP ? cur[i - BPP] : 0, bv = has_up ? up[i] : 0, cv = has_up && i >= BPP ? up[i - BPP] : 0;
    o[1 + i] = (uint8_t)st_png_filter_byte(ft, x, av, bv, cv);
  }
}

__global__ __launch_bounds__(256) void k_png_filter(PngFilterK a) {
  __shared__ unsigned s_sum[4][5];
  const long long row = blockIdx.x;
  if (row >= a.rows) return;
  const long long f = row / a.h;
  const int y = (int)(row - f * a.h), rb = a.rb;
  const uint8_t* __restrict__ cur = st_gl(a.frames[f]) + (size_t)y * rb;
  const uint8_t* __restrict__ up = cur - rb;   // read only below the first row
  uint8_t* __restrict__ o = a.filt + (size_t)f * a.stride + (size_t)y * (size_t)(1 + rb);
  if (a.bpp == 1) png_filter_row<1>(a, cur, up, y > 0, o, s_sum);
  else if (a.bpp == 3) png_filter_row<3>(a, cur, up, y > 0, o, s_sum);
  else png_filter_row<4>(a, cur, up, y > 0, o, s_sum);
}

struct PngDeflateK {
  const uint8_t* filt;
  uint8_t* slots;
  unsigned* clen;      // per piece: its chunk's bytes
  uint32_t* adler;     // per piece: sum of the bytes, sum of (L - i) * byte i, both mod 65521
  size_t stride, fb, slot_bytes;
  int pieces;
};

// The tokens that begin in [lo, hi) of the piece d[0, L): s is the start of the run lo lies in, nb the first run boundary at or
// after hi (L when there is none).  f(token, byte) in position order.
template <class F>
__device__ __forceinline__ void png_walk(const uint8_t* d, int lo, int hi, int s, int nb, F f) {
  int pos = lo;
  while (pos < hi) {
    int e = pos + 1;
    while (e < hi && d[e] == d[e - 1]) ++e;
    const int end = e < hi ? e : nb;   // where the run ends, in this stretch or beyond it
    const int R = end - s, stop = end < hi ? end : hi;
    const int byte = d[pos];
    for (int i = pos; i < stop; ++i) {
      const int tok = st_png_token(i - s, R);
      if (tok) f(tok, byte);
    }
    pos = stop;
    s = end;
  }
}

__device__ __forceinline__ void png_put(uint32_t* bits, unsigned pos, unsigned v, int n) {
  if (n == 0) return;
  const u64 vv = (u64)v << (pos & 31u);
  atomicOr(&bits[pos >> 5], (uint32_t)vv);
  if (vv >> 32) atomicOr(&bits[(pos >> 5) + 1], (uint32_t)(vv >> 32));
}

__global__ __launch_bounds__(256) void k_png_deflate(PngDeflateK a) {
  __shared__ uint4 s_data4[kPngPiece / 16];
  __shared__ uint32_t s_bits[kBitWords];
  __shared__ uint32_t s_freq[kPngLitLen + 2];
  __shared__ StPngHuffWork s_wk;
  __shared__ StPngBlockTables s_tb;
  __shared__ uint32_t s_crc[256];
  __shared__ int s_last[256], s_first[256];
  __shared__ uint32_t s_scan[256];
  __shared__ u64 s_red[2][256];
  __shared__ int s_m;
  const int tid = threadIdx.x;
  const size_t pc = blockIdx.x;
  const size_t f = pc / (size_t)a.pieces;
  const int p = (int)(pc - f * (size_t)a.pieces);
  const int L = st_png_piece_len(a.fb, p);
  const uint8_t* d = reinterpret_cast<const uint8_t*>(s_data4);
  {
    // the frames are 16 bytes apart at least and a piece is a multiple of 16: whole uint4, up to 15 bytes past the piece
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(a.filt + f * a.stride + (size_t)p * kPngPiece);
    for (int i = tid; i < (L + 15) / 16; i += 256) s_data4[i] = src[i];
  }
  for (int i = tid; i < kBitWords; i += 256) s_bits[i] = 0;
  for (int i = tid; i < kPngLitLen + 2; i += 256) s_freq[i] = i == 256 ? 1u : 0u;   // the end of the block
  s_crc[tid] = st_crc_table_entry((uint32_t)tid);
  if (tid == 0) s_m = 0;
  __syncthreads();

  // 1. run boundaries of the thread's stretch, and the piece's Adler sums
  const int lo = tid * kStretch < L ? tid * kStretch : L, hi = lo + kStretch < L ? lo + kStretch : L;
  int last = -1, first = L;
  u64 asum = 0, bsum = 0;
  for (int i = lo; i < hi; ++i) {
    const unsigned v = d[i];
    if (i == 0 || d[i - 1] != v) {
      last = i;
      first = first < L ? first : i;
    }
    asum += v;
    bsum += (u64)(unsigned)(L - i) * v;
  }
  s_last[tid] = last;
  s_first[tid] = first;
  s_red[0][tid] = asum;
  s_red[1][tid] = bsum;
  __syncthreads();
  for (int dd = 128; dd > 0; dd >>= 1) {
    if (tid < dd) {
      s_red[0][tid] += s_red[0][tid + dd];
      s_red[1][tid] += s_red[1][tid + dd];
    }
    __syncthreads();
  }
  if (tid == 0) {
    a.adler[2 * pc] = (uint32_t)(s_red[0][0] % kAdlerMod);
    a.adler[2 * pc + 1] = (uint32_t)(s_red[1][0] % kAdlerMod);
  }
  int s0 = lo, nb = L;   // the run the stretch begins in; the first boundary behind the stretch
  if (lo < hi) {
    if (!(lo == 0 || d[lo - 1] != d[lo]))
      for (int u = tid - 1; u >= 0; --u)   // position 0 is a boundary, so the search ends
        if (s_last[u] >= 0) {
          s0 = s_last[u];
          break;
        }
    for (int u = tid + 1; u < 256; ++u)
      if (s_first[u] < L) {
        nb = s_first[u];
        break;
      }
  }

  // 2. the symbol counts
  png_walk(d, lo, hi, s0, nb, [&](int tok, int byte) {
    int nbits, extra;
    atomicAdd(&s_freq[tok == 1 ? byte : st_png_len_symbol(tok, &nbits, &extra)], 1u);
  });
  __syncthreads();

  // 3. the codes.  All threads: every counted symbol's place among the others by (count, symbol) -- a total order, so this is the
  // order any sort gives --, the leaves' depths, the lengths dealt out, the canonical codes, the counts of the lengths sent and the
  // header's bit offsets.  One thread: the merges (two queue heads in registers), the folding and the code-length code.
  uint32_t* sx = reinterpret_cast<uint32_t*>(&s_red[0][0]);   // the Adler sums are out: 1024 words of scratch
  constexpr int kXDeep = 288, kXHlit = 289, kXMade = 290, kXTop = 291, kXClf = 296, kXFirst = 320, kXEnd = 344;
  for (int i = tid; i < kXEnd; i += 256) sx[i] = i == kXHlit ? 257u : 0u;   // [0, 288): leaves per depth
  for (int i = tid; i < kPngLitLen + 2; i += 256) s_tb.len[i] = 0;
  for (int i = tid; i < kPngLitLen; i += 256) {
    const uint32_t fi = s_freq[i];
    if (!fi) continue;
    int rank = 0;
    for (int j = 0; j < kPngLitLen; ++j) {
      const uint32_t fj = s_freq[j];
      rank += fj && (fj < fi || (fj == fi && j < i));
    }
    s_wk.order[rank] = (uint16_t)i;
    s_wk.weight[rank] = fi;
    atomicAdd(&s_m, 1);
  }
  __syncthreads();
  const int m = s_m;   // at least one literal and the end of the block: m >= 2
  if (tid == 0) sx[kXMade] = (uint32_t)st_png_huff_merge(&s_wk, m);
  __syncthreads();
  {
    const int root = (int)sx[kXMade] - 1;
    for (int k = tid; k < m; k += 256) {
      int node = k, dep = 0;
      while (node != root && dep < kPngLitLen) {   // (a leaf is at most m - 1 deep)
        node = s_wk.parent[node];
        ++dep;
      }
      atomicAdd(&sx[dep], 1u);
      atomicMax(&sx[kXDeep], (uint32_t)dep);
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int deepest = (int)sx[kXDeep];
    for (int i = 0; i <= (deepest > 16 ? deepest : 16); ++i) s_wk.count[i] = (uint16_t)sx[i];
    sx[kXTop] = (uint32_t)st_png_huff_fold(&s_wk, deepest, 15);
    st_png_huff_first(s_wk.count, 15, sx + kXFirst);
  }
  __syncthreads();
  {
    const int top = (int)sx[kXTop];
    for (int k = tid; k < m; k += 256) s_tb.len[s_wk.order[k]] = (uint8_t)st_png_huff_deal(&s_wk, top, k);
  }
  __syncthreads();
  for (int i = tid; i < kPngLitLen; i += 256) {
    const int len = s_tb.len[i];
    unsigned code = 0;
    if (len) {
      unsigned same = 0;   // lower-numbered symbols of this length
      for (int j = 0; j < i; ++j) same += s_tb.len[j] == len;
      code = st_png_rev(sx[kXFirst + len] + same, len);
      atomicAdd(&sx[kXClf + len], 1u);
      if (i >= 257) atomicMax(&sx[kXHlit], (uint32_t)(i + 1));
    }
    s_tb.code[i] = (uint16_t)code;
  }
  __syncthreads();
  if (tid == 0) {
    const int hlit = (int)sx[kXHlit];
    sx[kXClf] = (uint32_t)(hlit - m);   // the lengths sent that are zero
    sx[kXClf + 1] += 1u;                // the distance code 0, one bit
    st_png_block_cl(&s_wk, sx + kXClf, hlit, &s_tb);
  }
  __syncthreads();
  // the lengths sent -- hlit of them and the distance length -- two per thread: their bits, and the bits in front of them
  const int hlit = s_tb.hlit;
  unsigned hsym[2], hbits[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int e = 2 * tid + q;
    hsym[q] = e < hlit ? s_tb.len[e] : 1u;
    hbits[q] = e <= hlit ? s_tb.cl_len[hsym[q]] : 0u;
  }
  s_scan[tid] = hbits[0] + hbits[1];
  __syncthreads();
  uint32_t hbefore = 17u + 3u * (uint32_t)s_tb.hclen, header_bits = hbefore;
  for (int u = 0; u < 256; ++u) {
    const uint32_t v = s_scan[u];
    hbefore += u < tid ? v : 0u;
    header_bits += v;
  }
  __syncthreads();   // s_scan is used again below

  // 4. where the thread's tokens go
  uint32_t mine = 0;
  png_walk(d, lo, hi, s0, nb, [&](int tok, int byte) {
    if (tok == 1) {
      mine += s_tb.len[byte];
    } else {
      int nbits, extra;
      const int sym = st_png_len_symbol(tok, &nbits, &extra);
      mine += s_tb.len[sym] + nbits + 1;
    }
  });
  s_scan[tid] = mine;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int u = 0; u < 256; ++u) {
    const uint32_t v = s_scan[u];
    before += u < tid ? v : 0u;
    all += v;
  }
  const uint32_t block_bits = header_bits + all + s_tb.len[256];
  const uint32_t coded_bytes = st_png_coded_bytes(block_bits);
  const bool coded = coded_bytes < (uint32_t)(5 + L);   // decided before anything is written

  // 5. the bits
  if (coded) {
    unsigned at = header_bits + before;
    png_walk(d, lo, hi, s0, nb, [&](int tok, int byte) {
      if (tok == 1) {
        png_put(s_bits, at, s_tb.code[byte], s_tb.len[byte]);
        at += s_tb.len[byte];
      } else {
        int nbits, extra;
        const int sym = st_png_len_symbol(tok, &nbits, &extra);
        png_put(s_bits, at, s_tb.code[sym], s_tb.len[sym]);
        png_put(s_bits, at + s_tb.len[sym], (unsigned)extra, nbits);
        at += s_tb.len[sym] + nbits + 1;   // and one zero bit: distance code 0
      }
    });
    png_put(s_bits, hbefore, s_tb.cl_code[hsym[0]], (int)hbits[0]);
    png_put(s_bits, hbefore + hbits[0], s_tb.cl_code[hsym[1]], (int)hbits[1]);
    if (tid == 0) {
      unsigned hp = 0;
      st_png_block_header_front(s_tb, [&](unsigned v, int n) {
        png_put(s_bits, hp, v, n);
        hp += n;
      });
      png_put(s_bits, header_bits + all, s_tb.code[256], s_tb.len[256]);
      // the empty stored block: three zero bits, zeros up to the byte, 00 00 FF FF
      png_put(s_bits, (coded_bytes - 2) * 8, 0xffffu, 16);
    }
  }
  __syncthreads();

  // 6. the chunk: length, "IDAT", (the zlib header,) the data, the CRC of type and data
  const int zl = p == 0 ? 2 : 0;
  const uint32_t dlen = (uint32_t)zl + (coded ? coded_bytes : (uint32_t)(5 + L));
  const int mlen = 4 + (int)dlen;
  const uint8_t* cb = reinterpret_cast<const uint8_t*>(s_bits);
  auto msg_byte = [&](int j) -> unsigned {
    if (j < 4) return j == 0 ? 'I' : j == 1 ? 'D' : j == 2 ? 'A' : 'T';
    j -= 4;
    if (j < zl) return j == 0 ? 0x78u : 0x01u;
    j -= zl;
    if (coded) return cb[j];
    if (j < 5) return j == 0 ? 0u : j == 1 ? (unsigned)L & 0xffu : j == 2 ? (unsigned)L >> 8 : j == 3 ? ~(unsigned)L & 0xffu : (~(unsigned)L >> 8) & 0xffu;
    return d[j - 5];
  };
  uint8_t* __restrict__ slot = a.slots + pc * a.slot_bytes;   // 12 + dlen <= slot_bytes: the piece stored is the longest
  // type, zlib header and stored header bytewise; behind them the body -- the coded bits or the piece itself -- as whole dwords
  // from LDS to an address of any alignment, its last bytes bytewise
  const int head = 4 + zl + (coded ? 0 : 5), body = mlen - head;
  const uint8_t* bb = coded ? cb : d;
  const uint32_t* bw = reinterpret_cast<const uint32_t*>(bb);
  for (int j = tid; j < head; j += 256) slot[4 + j] = (uint8_t)msg_byte(j);
  u32u* __restrict__ body_dst = reinterpret_cast<u32u*>(slot + 4 + head);
  for (int i = tid; i < body / 4; i += 256) body_dst[i] = bw[i];
  for (int j = (body & ~3) + tid; j < body; j += 256) slot[4 + head + j] = bb[j];
  // The CRC of zeros followed by the message is the message's, so the message is right-aligned in 256 segments of 129 bytes;
  // a segment's remainder times x^(8 * bytes behind it) is its share.  The register starts as all ones: the first four bytes
  // are complemented instead.
  const int pad = 256 * kCrcSeg - mlen;
  uint32_t c = 0;
  for (int q = tid * kCrcSeg; q < (tid + 1) * kCrcSeg; ++q) {
    const int j = q - pad;
    if (j < 0) continue;
    const unsigned v = j < head ? msg_byte(j) ^ (j < 4 ? 0xffu : 0u) : (unsigned)bb[j - head];
    c = s_crc[(c ^ v) & 0xffu] ^ (c >> 8);
  }
  c = st_crc_mul(c, st_crc_x8n((uint32_t)(kCrcSeg * (255 - tid))));
  s_scan[tid] = c;
  __syncthreads();
  for (int dd = 128; dd > 0; dd >>= 1) {
    if (tid < dd) s_scan[tid] ^= s_scan[tid + dd];
    __syncthreads();
  }
  if (tid < 4) {
    slot[tid] = (uint8_t)(dlen >> (24 - 8 * tid));
    slot[4 + mlen + tid] = (uint8_t)((s_scan[0] ^ 0xffffffffu) >> (24 - 8 * tid));
  }
  if (tid == 0) a.clen[pc] = 12u + dlen;
}

struct PngLayoutK {
  const unsigned* clen;
  u64* poff;   // per piece: its chunk's place in the packed streams
  u64* offs;   // n + 1: the streams' places
  size_t total;
  int pieces;
};

// One workgroup: thread t sums a contiguous share of the chunk lengths, the shares are added up, every chunk gets the sum of
// those in front of it plus the 33 bytes in front of and the 33 behind each earlier frame.
__global__ __launch_bounds__(1024) void k_png_enc_layout(PngLayoutK a) {
  __shared__ u64 s_part[1024];
  const size_t tid = threadIdx.x;
  const size_t per = (a.total + 1023) / 1024;
  const size_t lo = tid * per < a.total ? tid * per : a.total, hi = lo + per < a.total ? lo + per : a.total;
  u64 sum = 0;
  for (size_t i = lo; i < hi; ++i) sum += a.clen[i];
  s_part[tid] = sum;
  __syncthreads();
  u64 at = 0;
  for (size_t u = 0; u < tid; ++u) at += s_part[u];
  const u64 fixed = (u64)(kPngHeadBytes + kPngTailBytes);
  for (size_t i = lo; i < hi; ++i) {
    const size_t f = i / (size_t)a.pieces;
    const u64 start = at + fixed * f;   // of the frame, when i is its first piece
    if (i == f * (size_t)a.pieces) a.offs[f] = start;
    a.poff[i] = start + kPngHeadBytes;
    at += a.clen[i];
  }
  if (hi == a.total && lo < hi) a.offs[a.total / (size_t)a.pieces] = at + fixed * (a.total / (size_t)a.pieces);
}

struct PngPackK {
  const uint8_t* slots;
  const unsigned* clen;
  const uint32_t* adler;
  const u64* poff;
  uint8_t* blob;
  size_t slot_bytes, blob_bytes, fb;
  int pieces;
  uint8_t head[kPngHeadBytes];
};

__global__ __launch_bounds__(256) void k_png_enc_pack(PngPackK a) {
  const int tid = threadIdx.x;
  const size_t pc = blockIdx.x;
  const size_t f = pc / (size_t)a.pieces;
  const int p = (int)(pc - f * (size_t)a.pieces);
  const u64 at = a.poff[pc];
  const unsigned len = a.clen[pc];
  if (at + len + kPngTailBytes > a.blob_bytes || at < (u64)kPngHeadBytes) return;   // every store below stays inside the blob
  uint8_t* __restrict__ dst = a.blob + at;
  const uint8_t* __restrict__ src = a.slots + pc * a.slot_bytes;   // 16-byte aligned
  const unsigned words = len / 4;
  for (unsigned j = tid; j < words; j += 256) reinterpret_cast<u32u*>(dst)[j] = reinterpret_cast<const uint32_t*>(src)[j];
  for (unsigned j = words * 4 + tid; j < len; j += 256) dst[j] = src[j];
  if (p == 0 && tid < kPngHeadBytes) dst[tid - kPngHeadBytes] = a.head[tid];
  if (p == a.pieces - 1 && tid == 0) {
    // Adler-32 of the frame from its pieces' sums: a piece of L bytes moves b on by L * a + its own weighted sum
    uint32_t sa = 1, sb = 0;
    for (int q = 0; q < a.pieces; ++q) {
      const size_t i = f * (size_t)a.pieces + q;
      const uint32_t L = (uint32_t)st_png_piece_len(a.fb, q);
      sb = (sb + sa * L % kAdlerMod + a.adler[2 * i + 1]) % kAdlerMod;
      sa = (sa + a.adler[2 * i]) % kAdlerMod;
    }
    const uint32_t ad = sb << 16 | sa;
    uint8_t t[kPngTailBytes] = {0, 0, 0, 9, 'I', 'D', 'A', 'T', 0x01, 0x00, 0x00, 0xFF, 0xFF, (uint8_t)(ad >> 24), (uint8_t)(ad >> 16), (uint8_t)(ad >> 8),
                                (uint8_t)ad, 0, 0, 0, 0, 0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
    uint32_t c = 0xffffffffu;
    for (int j = 4; j < 17; ++j) {
      c ^= t[j];
      for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    c ^= 0xffffffffu;
    t[17] = (uint8_t)(c >> 24); t[18] = (uint8_t)(c >> 16); t[19] = (uint8_t)(c >> 8); t[20] = (uint8_t)c;
    for (int j = 0; j < kPngTailBytes; ++j) dst[len + j] = t[j];
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
    return st_set_error(ctx, ST_ERR_OOM, "png_encode: hipMalloc(%zu) for %s failed: %s", bytes, what, hipGetErrorString(e));
  }
  *cap = want + want / 4;
  return ST_OK;
}

}  // namespace

struct st_png_enc_state {
  uint8_t* blob = nullptr;   // the packed streams of the last call
  size_t blob_cap = 0;
  u64* offs = nullptr;       // n + 1 offsets into it
  size_t offs_cap = 0;
  std::vector<u64> offs_host;
  uint8_t* pin = nullptr;
  size_t pin_cap = 0;
  int n = -1;                // streams to fetch; -1: none
};

void st_png_enc_release(st_ctx* ctx) {
  st_png_enc_state* s = ctx->png_enc;
  if (!s) return;
  if (s->blob) (void)hipFree(s->blob);
  if (s->offs) (void)hipFree(s->offs);
  if (s->pin) (void)hipHostFree(s->pin);
  delete s;
  ctx->png_enc = nullptr;
}

ST_EXPORT int st_png_encode_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int c, int filter) {
  ST_TRY(st_enter(ctx));
  // every refusal comes before the state is touched: the previous call's streams stay fetchable
  if (n < 1) return st_set_error(ctx, ST_ERR_INVALID, "png_encode: n = %d (at least one frame)", n);
  char msg[160];
  const int chk = st_png_enc_check(h, w, c, filter, msg, sizeof msg);
  if (chk != ST_OK) return st_set_error(ctx, chk, "png_encode: %s", msg);
  if (!frames_dev) return st_set_error(ctx, ST_ERR_INVALID, "png_encode: null frame table");
  ST_TRY(st_check_rows(ctx, "png_encode: frame %d is a null pointer", n, false, frames_dev));
  StPngEncGeom g;
  st_png_enc_geom(h, w, c, &g);
  const long long rows = (long long)n * h, total = (long long)n * g.pieces;
  if (rows > INT_MAX || total > INT_MAX)
    return st_set_error(ctx, ST_ERR_UNSUPPORTED, "png_encode: %lld rows and %lld pieces in one call (at most 2^31 - 1 of either)", rows, total);
  if (!ctx->png_enc) ctx->png_enc = new st_png_enc_state();
  st_png_enc_state* s = ctx->png_enc;
  s->n = -1;   // from here on a call that fails leaves nothing to fetch
  const size_t bound = (size_t)st_png_encode_bound(h, w, c);
  ST_TRY(grow(ctx, &s->blob, &s->blob_cap, (size_t)n * bound, "the streams"));
  ST_TRY(grow(ctx, &s->offs, &s->offs_cap, (size_t)n + 1, "the stream offsets"));

  const size_t longest = g.fb < (size_t)kPngPiece ? g.fb : (size_t)kPngPiece;
  const size_t slot_bytes = (12 + 2 + 5 + longest + 15) / 16 * 16;
  const size_t fbytes = (size_t)n * g.stride, sbytes = (size_t)total * slot_bytes, lbytes = sizeof(unsigned) * (size_t)total;
  const size_t abytes = 2 * sizeof(uint32_t) * (size_t)total, pbytes = sizeof(u64) * (size_t)total;
  const uint8_t** d_frames;
  ST_TRY(st_upload_tables(ctx, n, st_align_up(fbytes) + st_align_up(sbytes) + st_align_up(lbytes) + st_align_up(abytes) + st_align_up(pbytes),
                          frames_dev, &d_frames));
  uint8_t* d_filt = (uint8_t*)st_ws_alloc(ctx, fbytes);
  uint8_t* d_slots = (uint8_t*)st_ws_alloc(ctx, sbytes);
  unsigned* d_clen = (unsigned*)st_ws_alloc(ctx, lbytes);
  uint32_t* d_adler = (uint32_t*)st_ws_alloc(ctx, abytes);
  u64* d_poff = (u64*)st_ws_alloc(ctx, pbytes);
  if (!d_filt || !d_slots || !d_clen || !d_adler || !d_poff) return st_set_error(ctx, ST_ERR_OOM, "png_encode: workspace exhausted");

  PngFilterK fk;
  fk.frames = d_frames; fk.filt = d_filt; fk.stride = g.stride; fk.rows = rows; fk.h = h; fk.rb = g.rb; fk.bpp = c; fk.filter = filter;
  {
    st_timed tm(ctx, ST_K_JPEG);
    hipLaunchKernelGGL(k_png_filter, dim3((unsigned)rows), dim3(256), 0, ctx->stream, fk);
    ST_HIP(ctx, hipGetLastError());
  }
  PngDeflateK dk;
  dk.filt = d_filt; dk.slots = d_slots; dk.clen = d_clen; dk.adler = d_adler; dk.stride = g.stride; dk.fb = g.fb; dk.slot_bytes = slot_bytes;
  dk.pieces = g.pieces;
  {
    st_timed tm(ctx, ST_K_JPEG);
    hipLaunchKernelGGL(k_png_deflate, dim3((unsigned)total), dim3(256), 0, ctx->stream, dk);
    ST_HIP(ctx, hipGetLastError());
  }
  PngLayoutK lk;
  lk.clen = d_clen; lk.poff = d_poff; lk.offs = s->offs; lk.total = (size_t)total; lk.pieces = g.pieces;
  {
    st_timed tm(ctx, ST_K_JPEG);
    hipLaunchKernelGGL(k_png_enc_layout, dim3(1), dim3(1024), 0, ctx->stream, lk);
    ST_HIP(ctx, hipGetLastError());
  }
  PngPackK pk;
  pk.slots = d_slots; pk.clen = d_clen; pk.adler = d_adler; pk.poff = d_poff; pk.blob = s->blob; pk.slot_bytes = slot_bytes;
  pk.blob_bytes = (size_t)n * bound; pk.fb = g.fb; pk.pieces = g.pieces;
  {
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    memcpy(pk.head, sig, 8);
    uint8_t ihdr[25] = {0, 0, 0, 13, 'I', 'H', 'D', 'R', (uint8_t)(w >> 24), (uint8_t)(w >> 16), (uint8_t)(w >> 8), (uint8_t)w,
                        (uint8_t)(h >> 24), (uint8_t)(h >> 16), (uint8_t)(h >> 8), (uint8_t)h, 8, (uint8_t)(c == 1 ? 0 : c == 3 ? 2 : 6), 0, 0, 0};
    uint32_t crc = 0xffffffffu;
    for (int j = 4; j < 21; ++j) crc = st_crc_table_entry((crc ^ ihdr[j]) & 0xffu) ^ (crc >> 8);
    crc ^= 0xffffffffu;
    ihdr[21] = (uint8_t)(crc >> 24); ihdr[22] = (uint8_t)(crc >> 16); ihdr[23] = (uint8_t)(crc >> 8); ihdr[24] = (uint8_t)crc;
    memcpy(pk.head + 8, ihdr, 25);
  }
  {
    st_timed tm(ctx, ST_K_JPEG);
    hipLaunchKernelGGL(k_png_enc_pack, dim3((unsigned)total), dim3(256), 0, ctx->stream, pk);
    ST_HIP(ctx, hipGetLastError());
  }
  s->n = n;
  return ST_OK;
}

ST_EXPORT int st_png_encode_fetch(st_ctx* ctx, uint8_t* const* bufs_host, size_t* sizes, size_t capacity) {
  ST_TRY(st_enter(ctx));
  st_png_enc_state* s = ctx->png_enc;
  if (!s || s->n < 0) return st_set_error(ctx, ST_ERR_INVALID, "png_encode_fetch: no st_png_encode_batch call to fetch from");
  if (!sizes) return st_set_error(ctx, ST_ERR_INVALID, "png_encode_fetch: null sizes");
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
  if (most > capacity) return st_set_error(ctx, ST_ERR_INVALID, "png_encode_fetch: a stream has %zu bytes, the buffers hold %zu", most, capacity);
  for (size_t i = 0; i < n; ++i)
    if (!bufs_host[i]) return st_set_error(ctx, ST_ERR_INVALID, "png_encode_fetch: buffer %zu is a null pointer", i);
  const size_t total = (size_t)s->offs_host[n];
  ST_TRY(st_pinned_grow(ctx, (void**)&s->pin, &s->pin_cap, total, "png_encode_fetch: cannot page-lock %zu bytes for the streams"));
  ST_HIP(ctx, hipMemcpyAsync(s->pin, s->blob, total, hipMemcpyDeviceToHost, ctx->stream));   // every stream in one copy
  ST_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n; ++i) memcpy(bufs_host[i], s->pin + s->offs_host[i], sizes[i]);
  return ST_OK;
}
