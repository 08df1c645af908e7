// The entropy decoder of ONE restart interval of a baseline JPEG scan, shared by the host (st_jpeg_coefficients_by_interval,
// st_jpeg_parse.cpp) and the device (k_jpeg_entropy_dec, st_jpeg_entropy.hip): __host__ __device__ inline functions that also
// compile as plain C++17, where the two qualifiers are defined away.  It restates st_jpeg_decode_scan's arithmetic -- the
// MSB-first bit reader with FF00 unstuffing and FFFF fill bytes, the 9-bit lookahead plus max-code walk, receive_extend, the
// DC prediction, the AC rules (0x00 ends the block, 0xF0 skips 16, a run past coefficient 63 is an error) and the de-zigzag
// -- for a byte range nobody vouches for.  Bounded by construction:
//   - no byte outside [begin, end) is read; past `end` (or at a marker inside the range) the reader feeds zero bits and counts
//     them, and a block that consumed a counted bit is ST_JE_DATA_ENDS;
//   - every table index is masked to the table's size, every coefficient index is checked to be <= 63 before the store;
//   - every block address comes from the interval's own MCU range and the frame's geometry, never from the stream, and the
//     range is clipped to the frame's MCU grid;
//   - the loops run over the known MCU and block counts and the AC loop strictly advances k, so nothing can spin.
#ifndef ST_JPEG_ENTROPY_H_
#define ST_JPEG_ENTROPY_H_

#include <stddef.h>
#include <stdint.h>

#include "st_jpeg_parse.h"

#ifndef __HIP__
#define __host__
#define __device__
#endif

// status of one interval
enum { ST_JE_OK = 0, ST_JE_BAD_DC = 1, ST_JE_BAD_AC = 2, ST_JE_RUN = 3, ST_JE_DATA_ENDS = 4 };

inline const char* st_jpeg_entropy_cause(int status) {
  switch (status) {
    case ST_JE_BAD_DC: return "bad DC code";
    case ST_JE_BAD_AC: return "bad AC code";
    case ST_JE_RUN: return "a run leaves the block";
    case ST_JE_DATA_ENDS: return "the data ends inside the interval";
    default: return "no error";
  }
}

// What the core needs of a frame: its MCU grid and, per component, sampling, blocks per row and the first block of its plane
// in the layout of st_jpeg_coefficients (component planes in SOF order, each in raster order).
struct StJpegScanGeom {
  int32_t ncomp, mcux, mcuy, restart_interval;
  int32_t hs[3], vs[3], bw[3];
  int32_t plane[3];   // first block of each component's plane
};

inline StJpegScanGeom st_jpeg_scan_geom(const StJpegHeader& hd) {
  StJpegScanGeom g = {};
  g.ncomp = hd.ncomp;
  g.mcux = hd.mcux;
  g.mcuy = hd.mcuy;
  g.restart_interval = hd.restart_interval;
  int32_t off = 0;
  for (int c = 0; c < hd.ncomp; ++c) {
    g.hs[c] = hd.hs[c];
    g.vs[c] = hd.vs[c];
    g.bw[c] = hd.bw[c];
    g.plane[c] = off;
    off += hd.bw[c] * hd.bh[c];
  }
  return g;
}

// The tables of one frame as its scan selects them: component c decodes with dc[c] and ac[c].
struct StJpegFrameTables {
  StJpegHuff dc[3], ac[3];
};

// MSB-first bit reader over [pos, end) of buf: a 64-bit buffer refilled bytewise, FF00 unstuffed, FFFF a fill byte.  At any
// other FF (a marker, or a lone FF at the end of the range) and past `end` it feeds zero bits and counts them in `fake`.
// WIDE (the device): bytes come from aligned 8-byte words, three in flight -- w0 and w1 are the 16 bytes from wbase, w2 the
// word behind them, requested when w0 was retired, so a word's latency is hidden behind eight bytes of decoding.  That needs buf
// 8-byte aligned and readable up to 16 bytes past `end`; a word's address is clamped to the word that holds `end`, and of
// what a word holds only bytes inside [pos, end) are ever looked at, so the range is honoured exactly as by the byte loads.
struct StJpegBits {
  const uint8_t* buf;
  uint32_t pos, end;
  uint64_t acc;
  int nbits, fake;
  uint64_t w0, w1, w2;
  uint32_t wbase, wlast;
};

template <bool WIDE>
__host__ __device__ inline uint64_t st_jpeg_bits_word(const StJpegBits& br, uint32_t at) {
  if (!WIDE) return 0;
  return *reinterpret_cast<const uint64_t*>(br.buf + (at < br.wlast ? at : br.wlast));
}

template <bool WIDE>
__host__ __device__ inline void st_jpeg_bits_open(StJpegBits& br, const uint8_t* buf, uint32_t begin, uint32_t end) {
  br.buf = buf; br.pos = begin; br.end = end < begin ? begin : end;
  br.acc = 0; br.nbits = 0; br.fake = 0;
  br.wbase = begin & ~7u;
  br.wlast = (br.end + 7u) & ~7u;
  br.w0 = st_jpeg_bits_word<WIDE>(br, br.wbase);
  br.w1 = st_jpeg_bits_word<WIDE>(br, br.wbase + 8);
  br.w2 = st_jpeg_bits_word<WIDE>(br, br.wbase + 16);
}

// byte p of buf, pos <= p < end (the reader asks for pos and pos + 1 only, and pos never goes back)
template <bool WIDE>
__host__ __device__ inline unsigned st_jpeg_bits_byte(StJpegBits& br, uint32_t p) {
  if (!WIDE) return br.buf[p];
  if (p - br.wbase >= 16u) {   // at most one word ahead of the window: p <= wbase + 17
    br.wbase += 8;
    br.w0 = br.w1;
    br.w1 = br.w2;
    br.w2 = st_jpeg_bits_word<WIDE>(br, br.wbase + 16);
  }
  const uint32_t o = (p - br.wbase) & 15u;
  return (unsigned)((o < 8 ? br.w0 : br.w1) >> (8 * (o & 7u))) & 0xffu;
}

template <bool WIDE>
__host__ __device__ inline void st_jpeg_bits_refill(StJpegBits& br) {
  while (br.nbits <= 56) {
    unsigned b = 0;
    if (br.fake == 0 && br.pos < br.end) {
      b = st_jpeg_bits_byte<WIDE>(br, br.pos);
      if (b == 0xFF) {
        const unsigned next = br.pos + 1 < br.end ? st_jpeg_bits_byte<WIDE>(br, br.pos + 1) : 0x100u;
        if (next == 0x00) br.pos += 2;                      // stuffed FF
        else if (next == 0xFF) { ++br.pos; continue; }      // fill byte (pos advances: the loop ends)
        else { b = 0; br.fake += 8; }                       // a marker, or the range ends: stay on it
      } else {
        ++br.pos;
      }
    } else {
      br.fake += 8;
    }
    br.acc = (br.acc << 8) | b;
    br.nbits += 8;
  }
}
// n in 1..16, at least n bits buffered
__host__ __device__ inline unsigned st_jpeg_bits_peek(const StJpegBits& br, int n) { return (unsigned)(br.acc >> (br.nbits - n)) & ((1u << n) - 1u); }

// next Huffman symbol, or -1 (no code of <= 16 bits matches); at least 16 bits must be buffered
__host__ __device__ inline int st_jpeg_next_symbol(StJpegBits& br, const StJpegHuff& t) {
  const unsigned e = t.look[st_jpeg_bits_peek(br, 9) & 511u];
  if (e) {
    br.nbits -= (int)(e >> 8);
    return (int)(e & 255u);
  }
  int l = 10;
  int code = (int)st_jpeg_bits_peek(br, 10);
  while (code > t.maxcode[l]) {   // l <= 16 < 18 inside the loop
    ++l;
    if (l > 16) return -1;
    code = (int)st_jpeg_bits_peek(br, l);
  }
  br.nbits -= l;
  return t.vals[(code + t.valoff[l]) & 255];
}

// `s` (1..15) more bits as a signed value (T.81 F.2.2.1: below 2^(s-1) is negative)
__host__ __device__ inline int st_jpeg_receive_extend(StJpegBits& br, int s) {
  const int v = (int)st_jpeg_bits_peek(br, s);
  br.nbits -= s;
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// position k of the zigzag scan -> index in the row-major block (T.81 figure A.6).  The decoder takes the 64 entries as a
// pointer (`zz`): the host hands it st_jpeg_zigzag(), the kernel a copy in LDS, where a lookup is not a trip to memory.
__host__ __device__ inline int st_jpeg_natural(int k) {
  static constexpr uint8_t nat[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                      41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                      30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return nat[k & 63];
}

struct StJpegZigzag { uint8_t nat[64]; };
inline StJpegZigzag st_jpeg_zigzag() {
  StJpegZigzag z;
  for (int k = 0; k < 64; ++k) z.nat[k] = (uint8_t)st_jpeg_natural(k);
  return z;
}

// MCUs mcu0 .. mcu0 + nmcu - 1 of the frame from bytes [begin, end) of buf into `coef` (the frame's coefficients, the layout
// of st_jpeg_coefficients; every block of the interval is zeroed before it is filled).  tabs: the frame's tables.  Returns an
// ST_JE_* status; on an error the interval's remaining blocks are left as they were.  WIDE: see StJpegBits; the host runs the
// byte loads (its buffers are neither aligned nor padded), the kernel the words.
template <bool WIDE = false>
__host__ __device__ inline int st_jpeg_decode_interval(const uint8_t* buf, uint32_t begin, uint32_t end, long long mcu0, int nmcu,
                                                       const StJpegScanGeom& g, const StJpegFrameTables* tabs, const uint8_t* zz, int16_t* coef) {
  const long long total = (long long)g.mcux * g.mcuy;
  if (mcu0 < 0 || mcu0 >= total) return ST_JE_OK;
  if (nmcu > total - mcu0) nmcu = (int)(total - mcu0);
  StJpegBits br;
  st_jpeg_bits_open<WIDE>(br, buf, begin, end);
  int pred[3] = {0, 0, 0};
  int my = (int)(mcu0 / g.mcux), mx = (int)(mcu0 % g.mcux);
  const int ncomp = g.ncomp < 3 ? (g.ncomp < 1 ? 1 : g.ncomp) : 3;
  for (int m = 0; m < nmcu; ++m) {
    for (int c = 0; c < ncomp; ++c) {
      const StJpegHuff& dct = tabs->dc[c];
      const StJpegHuff& act = tabs->ac[c];
      for (int v = 0; v < g.vs[c]; ++v)
        for (int hh = 0; hh < g.hs[c]; ++hh) {
          int16_t* blk = coef + ((size_t)g.plane[c] + (size_t)(my * g.vs[c] + v) * g.bw[c] + (size_t)(mx * g.hs[c] + hh)) * 64;
          for (int i = 0; i < 64; ++i) blk[i] = 0;
          st_jpeg_bits_refill<WIDE>(br);
          int s = st_jpeg_next_symbol(br, dct);
          if (s < 0 || s > 15) return ST_JE_BAD_DC;
          if (s) pred[c] += st_jpeg_receive_extend(br, s);
          blk[0] = (int16_t)pred[c];
          for (int k = 1; k < 64;) {
            st_jpeg_bits_refill<WIDE>(br);
            const int rs = st_jpeg_next_symbol(br, act);
            if (rs < 0) return ST_JE_BAD_AC;
            const int r = rs >> 4;
            s = rs & 15;
            if (s == 0) {
              if (r != 15) break;   // end of block
              k += 16;
              continue;
            }
            k += r;
            if (k > 63) return ST_JE_RUN;
            blk[zz[k & 63] & 63] = (int16_t)st_jpeg_receive_extend(br, s);
            ++k;
          }
          if (br.nbits < br.fake) return ST_JE_DATA_ENDS;
        }
    }
    if (++mx == g.mcux) { mx = 0; ++my; }
  }
  return ST_JE_OK;
}

// ---- what st_jpeg_decode_batch_gpu uploads for k_jpeg_entropy_dec (st_jpeg.hip fills it, st_jpeg_entropy.hip reads it) --------
// One frame of a sub-batch.  The offsets are bytes from the start of the sub-batch's upload; the frame's interval table holds
// `nint` (begin, end) uint32 pairs relative to the frame's first entropy-coded byte, which sits at `bytes_off`.
struct alignas(16) StJpegEntFrame {
  StJpegScanGeom geom;
  uint32_t nint;            // restart intervals
  uint32_t tables;          // index of the frame's StJpegFrameTables
  uint64_t intervals_off;   // 8-byte aligned
  uint64_t bytes_off;       // 16-byte aligned; nbytes + at least 16 bytes of padding belong to the frame
  uint32_t nbytes;          // entropy-coded bytes of the frame: no interval reaches further
  uint32_t blk_off;         // the frame's first block within the sub-batch's coefficients
};
static_assert(sizeof(StJpegEntFrame) == 96, "one frame record is 96 bytes");

struct StJpegEntArgs {
  const uint8_t* upload;              // the device copy of the sub-batch's upload
  const StJpegEntFrame* frames;       // nf records inside it
  const StJpegFrameTables* tables;    // the table sets inside it
  int16_t* coef;                      // the sub-batch's coefficients: 64 per block, natural order
  unsigned long long* status;         // minimum over the failed lanes of (stream << 32) | (interval << 4) | ST_JE_*; ~0: clean
  int nf, first_stream;               // frames of the sub-batch; the call's index of its first one
};
constexpr unsigned long long kStJpegEntClean = ~0ull;
constexpr int kStJpegEntLanes = 64;   // intervals per workgroup ("interval group")

// ---- decoding by subsequence (the iteration) -------------------------------------------------------------------
// A SEGMENT is a byte range decoded from a known state (a restart interval, or the whole scan of a stream without DRI); it is cut
// into subsequences of S raw bytes, one lane each.  Between two symbols the decoder's state is (p, c, z): p the next unread bit,
// c the block inside its MCU, z the zigzag position (0: a DC symbol is next), packed into one 64-bit word so that two lanes at
// the same bit hold the same word.  p is CANONICAL: it names the raw byte that holds the next data bit, and at a byte boundary
// the start of the next data byte, behind a stuffed 00 and behind fill FFs -- st_jsq_window computes it from the raw bytes alone,
// never from what a reader happened to buffer.  Bounded as the interval core above: no byte outside [.., seg_end) is read, table
// indices are masked, the coefficient index is checked, block addresses come from the block count and the geometry, and every
// symbol either advances p or (on fake bits, at the end of the data) advances z towards a block end, where the walk stops.
constexpr uint64_t kStJsqInvalid = 1ull << 63;   // an exit nobody may continue from: the next lane starts at its own guess
constexpr uint64_t kStJsqNever = ~0ull;          // "entered from": no state yet
constexpr int kStJsqDefaultSubseqBytes = 128;
constexpr int kStJsqDefaultMaxRounds = 64;

__host__ __device__ inline uint64_t st_jsq_pack(uint32_t b, int o, int c, int z) {
  return (uint64_t)b | ((uint64_t)(o & 7) << 32) | ((uint64_t)(c & 63) << 35) | ((uint64_t)(z & 63) << 41);
}

// blocks of one MCU
__host__ __device__ inline int st_jsq_mcu_blocks(const StJpegScanGeom& g) {
  const int ncomp = g.ncomp < 3 ? 1 : 3;
  int n = 0;
  for (int c = 0; c < ncomp; ++c) n += (g.hs[c] & 7) * (g.vs[c] & 7);
  return n < 1 ? 1 : (n > 63 ? 63 : n);
}

// subsequences of a segment of `len` bytes: at least one, so that an empty segment still has a lane to report it
__host__ __device__ inline uint32_t st_jsq_count(uint32_t len, uint32_t S) { return len == 0 ? 1u : (uint32_t)(((uint64_t)len + S - 1) / S); }

// where lane `at` (a raw offset inside the segment) guesses the first data bit of its subsequence: behind the 00 of an FF 00 pair
__host__ __device__ inline uint64_t st_jsq_guess(const uint8_t* buf, uint32_t seg_begin, uint32_t seg_end, uint32_t at) {
  if (at > seg_begin && at < seg_end && buf[at - 1] == 0xFF && buf[at] == 0x00) ++at;
  return st_jsq_pack(at, 0, 0, 0);
}

// The 40 data bits from the data byte at raw position `pos` on (MSB first; 7 bits of offset + a 16-bit code + 15 more bits is the
// longest a symbol reaches).  r[j]: the canonical raw position of data byte j -- fill bytes skipped BEFORE it is named; a
// position at a marker, at a lone FF before `end`, or at `end` stays there, and the bytes from it on are zero (`*nreal` counts
// the real ones in front).  WIDE (the device): the 16 raw bytes around `pos` come from two aligned 8-byte words loaded at once --
// one trip to memory per symbol instead of one per byte; only a window that needs more raw bytes (fill bytes, many stuffed
// FFs) loads bytes behind them singly.  That needs buf 8-byte aligned and readable up to 16 bytes past `end`, as the upload
// provides; a word's address is clamped to the word that holds `end`, and of what a word holds only bytes inside [.., end) are
// ever looked at, so the range is honoured exactly as by the byte loads.
template <bool WIDE>
__host__ __device__ inline uint64_t st_jsq_window(const uint8_t* buf, uint32_t pos, uint32_t end, uint32_t* r, int* nreal) {
  uint64_t w = 0;
  int n = 0;
  bool stuck = false;
  const uint32_t base = pos & ~7u;
  uint64_t w0 = 0, w1 = 0;
  if (WIDE) {
    const uint32_t last = (end + 7u) & ~7u;
    w0 = *reinterpret_cast<const uint64_t*>(buf + (base < last ? base : last));
    w1 = *reinterpret_cast<const uint64_t*>(buf + (base + 8u < last ? base + 8u : last));
  }
  // byte p of buf, pos <= p < end
  auto at = [&](uint32_t p) -> unsigned {
    const uint32_t d = p - base;
    if (WIDE && d < 16u) return (unsigned)((d < 8u ? w0 : w1) >> (8u * (d & 7u))) & 0xffu;
    return buf[p];
  };
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    if (!stuck)
      while (pos < end && end - pos > 1 && at(pos) == 0xFF && at(pos + 1) == 0xFF) ++pos;   // fill bytes (pos advances: the loop ends)
    r[j] = pos;
    unsigned v = 0;
    if (!stuck && pos < end) {
      v = at(pos);
      if (v != 0xFF) { ++pos; ++n; }
      else if (end - pos > 1 && at(pos + 1) == 0x00) { pos += 2; ++n; }   // stuffed FF
      else { v = 0; stuck = true; }                                       // a marker, or the range ends: stay on it
    } else {
      stuck = true;
    }
    w = (w << 8) | v;
  }
  *nreal = n;
  return w;
}

struct StJsqOut {
  uint64_t exit;       // kStJsqInvalid: a bad code, a run that leaves the block, or the data ended
  uint32_t blocks;     // blocks completed (one that consumed a fake bit is not)
  uint32_t dc[3];      // per component, the sum of the DC differences met (WRITE: dc_before included), modulo 2^32
};

// F_i and the write step in one body, so that both walk the same symbols.  From state `enter`, whole symbols while p lies before
// sub_end (`to_the_end`: the segment's last lane in the write step goes on until the segment's blocks are done, as the interval
// decoder does).  WRITE = false: counts and the exit state.  WRITE = true: stores too -- absolute DC values from dc_before and
// the AC coefficients, into the blocks blocks_before, blocks_before + 1, ... of the segment that starts at MCU mcu0, and stops
// at seg_blocks; an error met before that is the stream's, and the return value is its ST_JE_*.  The blocks must be zero already:
// a block may be filled by two lanes.  WIDE: see st_jsq_window; the host runs the byte loads, the kernels the words.
template <bool WRITE, bool WIDE = false>
__host__ __device__ inline int st_jsq_run(const uint8_t* buf, uint32_t seg_end, uint32_t sub_end, bool to_the_end, uint64_t enter, const StJpegScanGeom& g,
                                          const StJpegFrameTables* tabs, const uint8_t* zz, long long mcu0, uint32_t seg_blocks, uint32_t blocks_before,
                                          const uint32_t* dc_before, int16_t* coef, StJsqOut* out) {
  const int ncomp = g.ncomp < 3 ? 1 : 3;
  const int bpm = st_jsq_mcu_blocks(g);
  uint32_t b = (uint32_t)enter;
  int o = (int)(enter >> 32) & 7, c = (int)(enter >> 35) & 63, z = (int)(enter >> 41) & 63;
  if (c >= bpm) c = 0;
  out->blocks = 0;
  for (int i = 0; i < 3; ++i) out->dc[i] = WRITE ? dc_before[i] : 0u;
  out->exit = enter;
  int status = ST_JE_OK;
  bool fake = false;                 // the block in progress consumed a fake bit
  int16_t* blk = nullptr;
  uint32_t at_block = ~0u;
  const long long total_mcus = (long long)g.mcux * g.mcuy;
  while ((to_the_end || b < sub_end) && (!WRITE || blocks_before + out->blocks < seg_blocks)) {
    // the component of block c of the MCU
    int comp = 0, cc = c;
    while (comp < ncomp - 1 && cc >= (g.hs[comp] & 7) * (g.vs[comp] & 7)) { cc -= (g.hs[comp] & 7) * (g.vs[comp] & 7); ++comp; }
    if (WRITE && at_block != blocks_before + out->blocks) {
      at_block = blocks_before + out->blocks;
      const long long mcu = mcu0 + at_block / (uint32_t)bpm;
      if (mcu < 0 || mcu >= total_mcus) break;   // (seg_blocks is clipped to the frame: never taken)
      int bc = 0, bi = (int)(at_block % (uint32_t)bpm);
      while (bc < ncomp - 1 && bi >= (g.hs[bc] & 7) * (g.vs[bc] & 7)) { bi -= (g.hs[bc] & 7) * (g.vs[bc] & 7); ++bc; }
      const int hsb = (g.hs[bc] & 7) ? (g.hs[bc] & 7) : 1;
      const int my = (int)(mcu / g.mcux), mx = (int)(mcu % g.mcux);
      blk = coef + ((size_t)g.plane[bc] + (size_t)(my * g.vs[bc] + bi / hsb) * g.bw[bc] + (size_t)(mx * g.hs[bc] + bi % hsb)) * 64;
    }
    uint32_t r[5];
    int nreal;
    StJpegBits br;
    br.acc = st_jsq_window<WIDE>(buf, b, seg_end, r, &nreal);
    br.nbits = 40 - o;
    if (z == 0) {
      const int s = st_jpeg_next_symbol(br, tabs->dc[comp]);
      if (s < 0 || s > 15) { status = ST_JE_BAD_DC; break; }
      if (s) out->dc[comp] += (uint32_t)st_jpeg_receive_extend(br, s);
      if (WRITE) blk[0] = (int16_t)(uint16_t)out->dc[comp];
      z = 1;
    } else {
      const int rs = st_jpeg_next_symbol(br, tabs->ac[comp]);
      if (rs < 0) { status = ST_JE_BAD_AC; break; }
      const int run = rs >> 4, s = rs & 15;
      if (s == 0) {
        z = run != 15 ? 64 : z + 16;   // end of block / sixteen zeros
      } else {
        z += run;
        if (z > 63) { status = ST_JE_RUN; break; }
        const int v = st_jpeg_receive_extend(br, s);
        if (WRITE) blk[zz[z & 63] & 63] = (int16_t)v;
        ++z;
      }
    }
    const int used = 40 - br.nbits;   // o + the symbol's bits: 2 .. 38
    if (used > 8 * nreal) fake = true;
    const int j = used >> 3;
    b = j == 0 ? r[0] : (j == 1 ? r[1] : (j == 2 ? r[2] : (j == 3 ? r[3] : r[4])));
    o = used & 7;
    if (z >= 64) {   // the block ends
      if (fake) { status = ST_JE_DATA_ENDS; break; }
      z = 0;
      out->blocks++;
      if (++c >= bpm) c = 0;
    }
  }
  out->exit = status == ST_JE_OK ? st_jsq_pack(b, o, c, z) : kStJsqInvalid;
  return status;
}

// ---- what st_jpeg_decode_batch_gpu_split adds to the upload and keeps beside the coefficients (st_jpeg.hip fills it, ----------
// ---- st_jpeg_subseq.hip reads it).  A frame's segments are its StJpegEntFrame's intervals (`nint` of them; one for a stream
// without DRI); its lanes are numbered through its segments in order.
struct alignas(16) StJsqFrame {
  uint64_t subpre_off;   // nint + 1 uint32: subsequences in front of each segment, then the frame's total; 4-byte aligned
  uint32_t lane_off;     // the frame's first lane within the sub-batch
  uint32_t seg_off;      // the frame's first segment within the sub-batch
  uint32_t nlanes;       // subsequences of the frame
  uint32_t pad[3];
};
static_assert(sizeof(StJsqFrame) == 32, "one record is 32 bytes");

struct StJsqArgs {
  StJpegEntArgs ent;           // upload, frames, tables, coefficients, status word, nf, first_stream
  const StJsqFrame* sq;        // nf records
  uint64_t* exits[2];          // per lane: the exit state, ping-pong between round launches
  uint64_t* entered;           // per lane: the state its exit and counts were computed from; after the scan, the state the
                               // write step enters with (kStJsqInvalid: the chain is broken in front of the lane)
  uint32_t* counts;            // per lane: blocks, dc[3]; after the scan their exclusive prefix over the segment
  uint32_t* unconverged;       // per segment: 1 when the scan found a lane that did not enter from its predecessor's exit
  unsigned* changed;           // exits changed, one counter per round launch of a group
  uint32_t S;                  // subsequence bytes
};
constexpr int kStJsqLanes = 64;        // subsequences per workgroup
constexpr int kStJsqRoundsPerLaunch = 16;

#endif  // ST_JPEG_ENTROPY_H_
