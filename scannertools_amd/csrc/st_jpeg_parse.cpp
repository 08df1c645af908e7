// Baseline JPEG on the host: marker parser and Huffman decoder (stage 1 of the ImageDecoder op; the dense stages are the
// kernels of st_jpeg.hip).  Written from the format's definition (ITU-T T.81): SOF0, 8-bit samples, 8-bit quantisation tables,
// one scan holding every component.  Every read is bounded by the buffer's size; a stream that is not such a JPEG gets a
// status and a message, never a crash.  No state between calls.
#include "st_jpeg_parse.h"

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>

#include "scannertools_hip.h"
#include "st_jpeg_entropy.h"

#define ST_JPEG_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

int fail(char* msg, size_t msg_len, int status, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  if (msg && msg_len) vsnprintf(msg, msg_len, fmt, ap);
  va_end(ap);
  return status;
}

// position k of the zigzag scan -> index in the row-major block (T.81 figure A.6)
const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// canonical code assignment (T.81 annex C) into the lookahead / max-code form; false: the counts do not form a prefix code
bool build_huff(const uint8_t* bits /* [16] */, const uint8_t* vals, int nvals, StJpegHuff* t) {
  memset(t, 0, sizeof *t);
  memcpy(t->vals, vals, (size_t)nvals);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    t->valoff[l] = k - code;
    for (int i = 0; i < bits[l - 1]; ++i, ++code, ++k) {
      if (code >= (1 << l)) return false;
      if (l <= 9) {
        const int first = code << (9 - l), count = 1 << (9 - l);
        for (int j = 0; j < count; ++j) t->look[first + j] = (uint16_t)((l << 8) | vals[k]);
      }
    }
    t->maxcode[l] = bits[l - 1] ? code - 1 : -1;
    code <<= 1;
  }
  t->maxcode[0] = -1;
  t->maxcode[17] = 0x7fffffff;
  return true;
}

const char* sof_name(int m) {
  switch (m) {
    case 0xC1: return "extended sequential (SOF1)";
    case 0xC2: return "progressive (SOF2)";
    case 0xC3: return "lossless (SOF3)";
    case 0xC5: case 0xC6: case 0xC7: return "hierarchical (SOF5-7)";
    case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF: return "arithmetic-coded (SOF9-15)";
    default: return "unknown SOF";
  }
}

}  // namespace

int st_jpeg_parse_header(const uint8_t* buf, size_t size, StJpegHeader* hd, char* msg, size_t msg_len) {
  if (msg && msg_len) msg[0] = 0;
  memset(hd, 0, sizeof *hd);
  if (!buf || size < 4 || buf[0] != 0xFF || buf[1] != 0xD8)
    return fail(msg, msg_len, ST_ERR_INVALID, "not a JPEG stream: %s", size == 0 || !buf ? "empty buffer" : "no SOI marker at its start");
  int ids[3] = {0, 0, 0};
  bool have_sof = false, jfif = false, adobe = false;
  int adobe_transform = 0;
  size_t pos = 2;
  for (;;) {
    if (pos >= size || buf[pos] != 0xFF)
      return fail(msg, msg_len, ST_ERR_INVALID, pos >= size ? "truncated stream: it ends at byte %zu, before any scan" : "malformed stream: no marker at byte %zu", pos);
    while (pos < size && buf[pos] == 0xFF) ++pos;   // fill bytes
    if (pos >= size) return fail(msg, msg_len, ST_ERR_INVALID, "truncated stream: it ends inside a marker");
    const int m = buf[pos++];
    if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // TEM, stray RSTn: no segment
    if (m == 0x00 || m == 0xD8) return fail(msg, msg_len, ST_ERR_INVALID, "malformed stream: marker 0xFF%02X among the tables", m);
    if (m == 0xD9) return fail(msg, msg_len, ST_ERR_INVALID, "malformed stream: EOI before any scan");
    if (pos + 2 > size) return fail(msg, msg_len, ST_ERR_INVALID, "truncated stream: it ends inside the segment of marker 0xFF%02X", m);
    const size_t len = (size_t)be16(buf + pos);
    if (len < 2 || pos + len > size)
      return fail(msg, msg_len, ST_ERR_INVALID, "truncated stream: the segment of marker 0xFF%02X%s is cut short", m, m == 0xDA ? " (SOS)" : "");
    const uint8_t* seg = buf + pos + 2;
    const size_t n = len - 2;
    pos += len;
    if (m == 0xC0 || m == 0xC1) {
      if (n < 6) return fail(msg, msg_len, ST_ERR_INVALID, "malformed SOF segment");
      if (seg[0] != 8) return fail(msg, msg_len, ST_ERR_UNSUPPORTED, "%d-bit sample precision is not supported (8-bit only)", seg[0]);
      if (m == 0xC1) return fail(msg, msg_len, ST_ERR_UNSUPPORTED, "%s streams are not supported (baseline SOF0 only)", sof_name(m));
      if (have_sof) return fail(msg, msg_len, ST_ERR_INVALID, "malformed stream: two SOF segments");
      hd->h = be16(seg + 1);
      hd->w = be16(seg + 3);
      hd->ncomp = seg[5];
      if (hd->h == 0 || hd->w == 0) return fail(msg, msg_len, ST_ERR_INVALID, "malformed SOF segment: %d x %d image", hd->w, hd->h);
      if (hd->ncomp == 4) return fail(msg, msg_len, ST_ERR_UNSUPPORTED, "4 components (CMYK / YCCK) are not supported");
      if (hd->ncomp != 1 && hd->ncomp != 3) return fail(msg, msg_len, ST_ERR_UNSUPPORTED, "%d components are not supported (1 or 3)", hd->ncomp);
      if (n != 6 + 3 * (size_t)hd->ncomp) return fail(msg, msg_len, ST_ERR_INVALID, "malformed SOF segment: wrong length");
      for (int c = 0; c < hd->ncomp; ++c) {
        ids[c] = seg[6 + 3 * c];
        hd->hs[c] = seg[7 + 3 * c] >> 4;
        hd->vs[c] = seg[7 + 3 * c] & 15;
        hd->tq[c] = seg[8 + 3 * c];
        if (hd->hs[c] < 1 || hd->hs[c] > 4 || hd->vs[c] < 1 || hd->vs[c] > 4 || hd->tq[c] > 3)
          return fail(msg, msg_len, ST_ERR_INVALID, "malformed SOF segment: component %d", c);
      }
      have_sof = true;
    } else if (m >= 0xC2 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      return fail(msg, msg_len, ST_ERR_UNSUPPORTED, "%s streams are not supported (baseline SOF0 only)", sof_name(m));
    } else if (m == 0xCC) {
      return fail(msg, msg_len, ST_ERR_UNSUPPORTED, "arithmetic-coded streams are not supported (DAC segment)");
    } else if (m == 0xC4) {   // DHT: one or more tables
      size_t i = 0;
      while (i < n) {
        if (n - i < 17) return fail(msg, msg_len, ST_ERR_INVALID, "malformed DHT segment");
        const int tc = seg[i] >> 4, th = seg[i] & 15;
        int count = 0;
        for (int l = 0; l < 16; ++l) count += seg[i + 1 + l];
        if (tc > 1 || th > 3 || count > 256 || n - i - 17 < (size_t)count) return fail(msg, msg_len, ST_ERR_INVALID, "malformed DHT segment");
        StJpegHuff* t = tc ? &hd->ac[th] : &hd->dc[th];
        if (!build_huff(seg + i + 1, seg + i + 17, count, t)) return fail(msg, msg_len, ST_ERR_INVALID, "malformed DHT segment: not a prefix code");
        (tc ? hd->have_ac : hd->have_dc)[th] = true;
        i += 17 + (size_t)count;
      }
    } else if (m == 0xDB) {   // DQT: one or more tables, stored in zigzag order
      size_t i = 0;
      while (i < n) {
        const int pq = seg[i] >> 4, tq = seg[i] & 15;
        if (pq == 1) return fail(msg, msg_len, ST_ERR_UNSUPPORTED, "16-bit quantisation tables are not supported");
        if (pq > 1 || tq > 3 || n - i < 65) return fail(msg, msg_len, ST_ERR_INVALID, "malformed DQT segment");
        for (int k = 0; k < 64; ++k) hd->quant[tq][kNatural[k]] = seg[i + 1 + k];
        hd->have_q[tq] = true;
        i += 65;
      }
    } else if (m == 0xDD) {
      if (n != 2) return fail(msg, msg_len, ST_ERR_INVALID, "malformed DRI segment");
      hd->restart_interval = be16(seg);
    } else if (m == 0xE0) {
      if (n >= 5 && memcmp(seg, "JFIF", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (n >= 12 && memcmp(seg, "Adobe", 5) == 0) { adobe = true; adobe_transform = seg[11]; }
    } else if (m == 0xDA) {
      if (!have_sof) return fail(msg, msg_len, ST_ERR_INVALID, "malformed stream: SOS before SOF");
      if (n < 1) return fail(msg, msg_len, ST_ERR_INVALID, "malformed SOS segment");
      const int ns = seg[0];
      if (ns < 1 || ns > 4 || n != 4 + 2 * (size_t)ns) return fail(msg, msg_len, ST_ERR_INVALID, "malformed SOS segment");
      if (ns != hd->ncomp)
        return fail(msg, msg_len, ST_ERR_UNSUPPORTED, "multiple scans are not supported (the first scan holds %d of %d components)", ns, hd->ncomp);
      for (int c = 0; c < ns; ++c) {
        if (seg[1 + 2 * c] != ids[c]) return fail(msg, msg_len, ST_ERR_UNSUPPORTED, "scan components out of frame order are not supported");
        hd->td[c] = seg[2 + 2 * c] >> 4;
        hd->ta[c] = seg[2 + 2 * c] & 15;
        if (hd->td[c] > 3 || hd->ta[c] > 3) return fail(msg, msg_len, ST_ERR_INVALID, "malformed SOS segment: table selector");
        if (!hd->have_dc[hd->td[c]] || !hd->have_ac[hd->ta[c]] || !hd->have_q[hd->tq[c]])
          return fail(msg, msg_len, ST_ERR_INVALID, "malformed stream: component %d uses a table that was never defined", c);
      }
      if (seg[1 + 2 * ns] != 0 || seg[2 + 2 * ns] != 63 || seg[3 + 2 * ns] != 0)
        return fail(msg, msg_len, ST_ERR_INVALID, "malformed SOS segment: spectral selection / approximation in a baseline scan");
      hd->scan_pos = pos;
      break;
    }
    // anything else (APPn, COM, DNL, JPGn, reserved): skipped
  }
  if (hd->ncomp == 3) {
    // what the samples mean: JFIF says YCbCr; an Adobe segment names its transform; otherwise the ids 'R','G','B' mean RGB
    if (!jfif && adobe && adobe_transform != 1)
      return fail(msg, msg_len, ST_ERR_UNSUPPORTED, "Adobe colour transform %d is not supported (YCbCr only)", adobe_transform);
    if (!jfif && !adobe && ids[0] == 'R' && ids[1] == 'G' && ids[2] == 'B')
      return fail(msg, msg_len, ST_ERR_UNSUPPORTED, "RGB-coded streams are not supported (YCbCr only)");
    const int H = hd->hs[0], V = hd->vs[0];
    const bool chroma1 = hd->hs[1] == 1 && hd->vs[1] == 1 && hd->hs[2] == 1 && hd->vs[2] == 1;
    if (!chroma1 || !((H == 1 && V == 1) || (H == 2 && V == 1) || (H == 2 && V == 2)))
      return fail(msg, msg_len, ST_ERR_UNSUPPORTED, "sampling %dx%d,%dx%d,%dx%d is not supported (4:4:4, 4:2:2 and 4:2:0 only)", hd->hs[0],
                  hd->vs[0], hd->hs[1], hd->vs[1], hd->hs[2], hd->vs[2]);
    hd->mode = H == 1 ? ST_JPEG_444 : (V == 1 ? ST_JPEG_H2V1 : ST_JPEG_H2V2);
    hd->mcux = (hd->w + 8 * H - 1) / (8 * H);
    hd->mcuy = (hd->h + 8 * V - 1) / (8 * V);
  } else {
    hd->hs[0] = hd->vs[0] = 1;   // a one-component scan is not interleaved: its MCU is one block
    hd->mode = ST_JPEG_GRAY;
    hd->mcux = (hd->w + 7) / 8;
    hd->mcuy = (hd->h + 7) / 8;
  }
  for (int c = 0; c < hd->ncomp; ++c) {
    hd->bw[c] = hd->mcux * hd->hs[c];
    hd->bh[c] = hd->mcuy * hd->vs[c];
  }
  return ST_OK;
}

namespace {

// MSB-first bit reader over the entropy-coded segment: a 64-bit buffer refilled bytewise, FF00 unstuffed.  At a marker
// or the end of the buffer it feeds zero bits and counts them (`fake`); using one of those is the caller's error to report.
struct BitReader {
  const uint8_t* buf;
  size_t size, pos;
  uint64_t acc = 0;
  int nbits = 0, fake = 0;

  inline void refill() {
    while (nbits <= 56) {
      unsigned b = 0;
      if (fake == 0 && pos < size) {
        b = buf[pos];
        if (b == 0xFF) {
          if (pos + 1 < size && buf[pos + 1] == 0x00) pos += 2;            // stuffed FF
          else if (pos + 1 < size && buf[pos + 1] == 0xFF) { ++pos; continue; }   // fill byte
          else { b = 0; fake += 8; }                                        // a marker (or a lone FF at the end): stay on it
        } else {
          ++pos;
        }
      } else {
        fake += 8;
      }
      acc = (acc << 8) | b;
      nbits += 8;
    }
  }
  inline unsigned peek(int n) const { return (unsigned)(acc >> (nbits - n)) & ((1u << n) - 1u); }
  inline void skip(int n) { nbits -= n; }
  inline bool overrun() const { return nbits < fake; }
  void reset() { acc = 0; nbits = 0; fake = 0; }
};

// next Huffman symbol, or -1 (no code of <= 16 bits matches); at least 16 bits must be buffered
inline int next_symbol(BitReader& br, const StJpegHuff& t) {
  const unsigned e = t.look[br.peek(9)];
  if (e) {
    br.skip((int)(e >> 8));
    return (int)(e & 255u);
  }
  int l = 10;
  int code = (int)br.peek(10);
  while (code > t.maxcode[l]) {
    ++l;
    if (l > 16) return -1;
    code = (int)br.peek(l);
  }
  br.skip(l);
  return t.vals[(code + t.valoff[l]) & 255];
}

// `s` more bits as a signed value (T.81 F.2.2.1: below 2^(s-1) is negative)
inline int receive_extend(BitReader& br, int s) {
  const int v = (int)br.peek(s);
  br.skip(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

}  // namespace

int st_jpeg_decode_scan(const uint8_t* buf, size_t size, const StJpegHeader& hd, int16_t* coef, char* msg, size_t msg_len) {
  if (msg && msg_len) msg[0] = 0;
  BitReader br{buf, size, hd.scan_pos};
  int16_t* plane[3];
  size_t off = 0;
  for (int c = 0; c < hd.ncomp; ++c) {
    plane[c] = coef + off;
    off += st_jpeg_comp_blocks(hd, c) * 64;
  }
  int pred[3] = {0, 0, 0};
  const int ri = hd.restart_interval;
  long long mcu = 0;
  for (int my = 0; my < hd.mcuy; ++my)
    for (int mx = 0; mx < hd.mcux; ++mx, ++mcu) {
      if (ri > 0 && mcu > 0 && mcu % ri == 0) {
        // restart: drop the padding bits, expect RSTn (after optional fill bytes), reset the predictors
        if (br.overrun()) return fail(msg, msg_len, ST_ERR_INVALID, "truncated or corrupt scan: data ends before restart interval %lld", mcu / ri);
        size_t p = br.pos;
        while (p + 1 < size && buf[p] == 0xFF && buf[p + 1] == 0xFF) ++p;
        const int want = 0xD0 + (int)((mcu / ri - 1) & 7);
        if (p + 1 >= size || buf[p] != 0xFF || buf[p + 1] != want)
          return fail(msg, msg_len, ST_ERR_INVALID, "truncated or corrupt scan: no RST%d marker at MCU %lld", want - 0xD0, mcu);
        br.pos = p + 2;
        br.reset();
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < hd.ncomp; ++c) {
        const StJpegHuff& dct = hd.dc[hd.td[c]];
        const StJpegHuff& act = hd.ac[hd.ta[c]];
        for (int v = 0; v < hd.vs[c]; ++v)
          for (int hh = 0; hh < hd.hs[c]; ++hh) {
            int16_t* blk = plane[c] + ((size_t)(my * hd.vs[c] + v) * hd.bw[c] + (size_t)(mx * hd.hs[c] + hh)) * 64;
            memset(blk, 0, 128);
            br.refill();
            int s = next_symbol(br, dct);
            if (s < 0 || s > 15) return fail(msg, msg_len, ST_ERR_INVALID, "corrupt scan: bad DC code in MCU %lld", mcu);
            if (s) pred[c] += receive_extend(br, s);
            blk[0] = (int16_t)pred[c];
            for (int k = 1; k < 64;) {
              br.refill();
              const int rs = next_symbol(br, act);
              if (rs < 0) return fail(msg, msg_len, ST_ERR_INVALID, "corrupt scan: bad AC code in MCU %lld", mcu);
              const int r = rs >> 4;
              s = rs & 15;
              if (s == 0) {
                if (r != 15) break;   // end of block
                k += 16;
                continue;
              }
              k += r;
              if (k > 63) return fail(msg, msg_len, ST_ERR_INVALID, "corrupt scan: a run leaves the block in MCU %lld", mcu);
              blk[kNatural[k]] = (int16_t)receive_extend(br, s);
              ++k;
            }
            if (br.overrun())
              return fail(msg, msg_len, ST_ERR_INVALID, "truncated or corrupt scan: the data ends in MCU %lld of %lld", mcu, (long long)hd.mcux * hd.mcuy);
          }
      }
    }
  return ST_OK;
}

int st_jpeg_scan_intervals(const uint8_t* buf, size_t size, const StJpegHeader& hd, uint32_t* table, char* msg, size_t msg_len) {
  if (msg && msg_len) msg[0] = 0;
  const size_t need = st_jpeg_interval_count(hd);
  if (need == 0) return fail(msg, msg_len, ST_ERR_UNSUPPORTED, "no restart intervals: the stream has no DRI segment");
  if (size >= ((size_t)1 << 32)) return fail(msg, msg_len, ST_ERR_UNSUPPORTED, "no restart intervals: a stream of %zu bytes is too long (below 4 GiB only)", size);
  size_t pos = hd.scan_pos, begin = hd.scan_pos, k = 0;
  for (;;) {
    const uint8_t* p = pos < size ? (const uint8_t*)memchr(buf + pos, 0xFF, size - pos) : nullptr;
    size_t end = size;   // the end of the buffer ends the scan (a lone 0xFF as its last byte included)
    int m = -1;
    if (p && (size_t)(p - buf) + 1 < size) {
      pos = (size_t)(p - buf);
      m = p[1];
      if (m == 0x00) { pos += 2; continue; }   // stuffed FF
      if (m == 0xFF) { pos += 1; continue; }   // fill byte
      end = pos;
    }
    const bool rst = m >= 0xD0 && m <= 0xD7;
    if (rst && k + 1 < need && m != 0xD0 + (int)(k & 7))
      return fail(msg, msg_len, ST_ERR_INVALID, "truncated or corrupt scan: no RST%d marker after restart interval %zu (RST%d at byte %zu)", (int)(k & 7), k,
                  m - 0xD0, end);
    table[2 * k] = (uint32_t)begin;
    table[2 * k + 1] = (uint32_t)end;
    ++k;
    if (k == need) return ST_OK;   // what follows is ignored
    if (!rst)
      return fail(msg, msg_len, ST_ERR_INVALID, "truncated or corrupt scan: %zu of %zu restart intervals before %s", k, need,
                  m < 0 ? "the end of the buffer" : "another marker");
    pos = begin = end + 2;
  }
}

namespace {
void fill_info(const StJpegHeader& hd, st_jpeg_info* info) {
  info->h = hd.h;
  info->w = hd.w;
  info->channels = hd.ncomp;
  info->h_samp = hd.hs[0];
  info->v_samp = hd.vs[0];
  info->restart_interval = hd.restart_interval;
}
}  // namespace

ST_JPEG_EXPORT int st_jpeg_probe(const uint8_t* buf, size_t size, st_jpeg_info* info) {
  if (!info) return ST_ERR_INVALID;
  memset(info, 0, sizeof *info);
  StJpegHeader hd;
  const int st = st_jpeg_parse_header(buf, size, &hd, info->message, sizeof info->message);
  if (st == ST_OK) fill_info(hd, info);
  return st;
}

ST_JPEG_EXPORT int st_jpeg_scaled_size(int h, int w, int scale_denom, int* oh, int* ow) {
  const int d = scale_denom;
  if ((d != 1 && d != 2 && d != 4 && d != 8) || h < 1 || w < 1 || h > 65535 || w > 65535 || !oh || !ow) return ST_ERR_INVALID;
  *oh = (h + d - 1) / d;
  *ow = (w + d - 1) / d;
  return ST_OK;
}

ST_JPEG_EXPORT int st_jpeg_scaled_geometry(const uint8_t* buf, size_t size, int scale_denom, int S[3], int dw[3], int dh[3], st_jpeg_info* info) {
  st_jpeg_info local;
  if (!info) info = &local;
  memset(info, 0, sizeof *info);
  const int d = scale_denom;
  if ((d != 1 && d != 2 && d != 4 && d != 8) || !S || !dw || !dh)
    return fail(info->message, sizeof info->message, ST_ERR_INVALID, "scale_denom %d: 1, 2, 4 or 8, and no null pointer", d);
  StJpegHeader hd;
  const int st = st_jpeg_parse_header(buf, size, &hd, info->message, sizeof info->message);
  if (st != ST_OK) return st;
  fill_info(hd, info);
  st_jpeg_reduced_geom(hd, d, S, dw, dh);
  return ST_OK;
}

ST_JPEG_EXPORT int st_jpeg_coefficients(const uint8_t* buf, size_t size, int16_t* coef, size_t cap, uint16_t* quant, st_jpeg_info* info) {
  st_jpeg_info local;
  if (!info) info = &local;
  memset(info, 0, sizeof *info);
  StJpegHeader hd;
  int st = st_jpeg_parse_header(buf, size, &hd, info->message, sizeof info->message);
  if (st != ST_OK) return st;
  fill_info(hd, info);
  const size_t need = st_jpeg_blocks(hd) * 64;
  if (!coef || cap < need) return fail(info->message, sizeof info->message, ST_ERR_INVALID, "coef holds %zu values, the stream has %zu", coef ? cap : (size_t)0, need);
  st = st_jpeg_decode_scan(buf, size, hd, coef, info->message, sizeof info->message);
  if (st != ST_OK) return st;
  if (quant)
    for (int c = 0; c < hd.ncomp; ++c) memcpy(quant + 64 * c, hd.quant[hd.tq[c]], 128);
  return ST_OK;
}

ST_JPEG_EXPORT int st_jpeg_restart_intervals(const uint8_t* buf, size_t size, uint32_t* table, size_t cap, size_t* count, st_jpeg_info* info) {
  st_jpeg_info local;
  if (!info) info = &local;
  memset(info, 0, sizeof *info);
  if (count) *count = 0;
  StJpegHeader hd;
  const int st = st_jpeg_parse_header(buf, size, &hd, info->message, sizeof info->message);
  if (st != ST_OK) return st;
  fill_info(hd, info);
  const size_t need = st_jpeg_interval_count(hd);
  if (need == 0) return fail(info->message, sizeof info->message, ST_ERR_UNSUPPORTED, "no restart intervals: the stream has no DRI segment");
  if (count) *count = need;
  if (!table) return ST_OK;
  if (cap < need) return fail(info->message, sizeof info->message, ST_ERR_INVALID, "table holds %zu pairs, the stream has %zu restart intervals", cap, need);
  return st_jpeg_scan_intervals(buf, size, hd, table, info->message, sizeof info->message);
}

ST_JPEG_EXPORT int st_jpeg_coefficients_by_interval(const uint8_t* buf, size_t size, int16_t* coef, size_t cap, uint16_t* quant, st_jpeg_info* info) {
  st_jpeg_info local;
  if (!info) info = &local;
  memset(info, 0, sizeof *info);
  StJpegHeader hd;
  int st = st_jpeg_parse_header(buf, size, &hd, info->message, sizeof info->message);
  if (st != ST_OK) return st;
  fill_info(hd, info);
  const size_t need = st_jpeg_blocks(hd) * 64;
  if (!coef || cap < need) return fail(info->message, sizeof info->message, ST_ERR_INVALID, "coef holds %zu values, the stream has %zu", coef ? cap : (size_t)0, need);
  const size_t nint = st_jpeg_interval_count(hd);
  if (nint == 0) return fail(info->message, sizeof info->message, ST_ERR_UNSUPPORTED, "no restart intervals: the stream has no DRI segment");
  uint32_t* table = new (std::nothrow) uint32_t[2 * nint];
  StJpegFrameTables* tabs = new (std::nothrow) StJpegFrameTables;
  if (!table || !tabs) {
    delete[] table;
    delete tabs;
    return fail(info->message, sizeof info->message, ST_ERR_OOM, "out of host memory for %zu restart intervals", nint);
  }
  st = st_jpeg_scan_intervals(buf, size, hd, table, info->message, sizeof info->message);
  if (st == ST_OK) {
    for (int c = 0; c < hd.ncomp; ++c) {
      tabs->dc[c] = hd.dc[hd.td[c]];
      tabs->ac[c] = hd.ac[hd.ta[c]];
    }
    const StJpegScanGeom g = st_jpeg_scan_geom(hd);
    const StJpegZigzag zz = st_jpeg_zigzag();
    for (size_t k = 0; k < nint && st == ST_OK; ++k) {
      const int je = st_jpeg_decode_interval(buf, table[2 * k], table[2 * k + 1], (long long)k * hd.restart_interval, hd.restart_interval, g, tabs, zz.nat, coef);
      if (je != ST_JE_OK)
        st = fail(info->message, sizeof info->message, ST_ERR_INVALID, "corrupt scan: restart interval %zu of %zu: %s", k, nint, st_jpeg_entropy_cause(je));
    }
  }
  delete[] table;
  delete tabs;
  if (st != ST_OK) return st;
  if (quant)
    for (int c = 0; c < hd.ncomp; ++c) memcpy(quant + 64 * c, hd.quant[hd.tq[c]], 128);
  return ST_OK;
}

// ---- decoding by subsequence: the segment table and the CPU twin of st_jpeg_subseq.hip ------------------------
int st_jpeg_segments(const uint8_t* buf, size_t size, const StJpegHeader& hd, uint32_t* table, char* msg, size_t msg_len) {
  if (hd.restart_interval > 0) return st_jpeg_scan_intervals(buf, size, hd, table, msg, msg_len);
  if (msg && msg_len) msg[0] = 0;
  if (size >= ((size_t)1 << 32)) return fail(msg, msg_len, ST_ERR_UNSUPPORTED, "a stream of %zu bytes is too long (below 4 GiB only)", size);
  size_t pos = hd.scan_pos, end = size;   // the end of the buffer ends the scan (a lone 0xFF as its last byte included)
  while (pos < size) {
    const uint8_t* p = (const uint8_t*)memchr(buf + pos, 0xFF, size - pos);
    if (!p || (size_t)(p - buf) + 1 >= size) break;
    pos = (size_t)(p - buf);
    if (p[1] == 0x00) { pos += 2; continue; }   // stuffed FF
    if (p[1] == 0xFF) { pos += 1; continue; }   // fill byte
    end = pos;
    break;
  }
  table[0] = (uint32_t)hd.scan_pos;
  table[1] = (uint32_t)end;
  return ST_OK;
}

ST_JPEG_EXPORT int st_jpeg_scan_segments(const uint8_t* buf, size_t size, uint32_t* table, size_t cap, size_t* count, st_jpeg_info* info) {
  st_jpeg_info local;
  if (!info) info = &local;
  memset(info, 0, sizeof *info);
  if (count) *count = 0;
  StJpegHeader hd;
  const int st = st_jpeg_parse_header(buf, size, &hd, info->message, sizeof info->message);
  if (st != ST_OK) return st;
  fill_info(hd, info);
  const size_t need = st_jpeg_segment_count(hd);
  if (count) *count = need;
  if (!table) return ST_OK;
  if (cap < need) return fail(info->message, sizeof info->message, ST_ERR_INVALID, "table holds %zu pairs, the stream has %zu segments", cap, need);
  return st_jpeg_segments(buf, size, hd, table, info->message, sizeof info->message);
}

ST_JPEG_EXPORT int st_jpeg_coefficients_by_subsequence(const uint8_t* buf, size_t size, const st_jpeg_split_opts* opts, int16_t* coef, size_t cap,
                                                       uint16_t* quant, st_jpeg_info* info, int* rounds) {
  st_jpeg_info local;
  if (!info) info = &local;
  memset(info, 0, sizeof *info);
  if (rounds) *rounds = 0;
  const int S = opts && opts->subseq_bytes ? opts->subseq_bytes : kStJsqDefaultSubseqBytes;
  const int R = opts && opts->max_rounds ? opts->max_rounds : kStJsqDefaultMaxRounds;
  if (S < 8 || S > 4096 || S % 8 != 0 || R < 0)
    return fail(info->message, sizeof info->message, ST_ERR_INVALID, "subseq_bytes %d / max_rounds %d: a multiple of 8 in 8..4096, and no negative cap", S, R);
  StJpegHeader* hdp = new (std::nothrow) StJpegHeader;
  StJpegFrameTables* tabs = new (std::nothrow) StJpegFrameTables;
  uint32_t* table = nullptr;
  uint64_t* words = nullptr;   // per lane: exit, next exit, entered-from
  StJsqOut* outs = nullptr;
  int st = ST_OK;
  if (!hdp || !tabs) st = fail(info->message, sizeof info->message, ST_ERR_OOM, "out of host memory");
  if (st == ST_OK) st = st_jpeg_parse_header(buf, size, hdp, info->message, sizeof info->message);
  size_t need = 0, nseg = 0;
  if (st == ST_OK) {
    fill_info(*hdp, info);
    need = st_jpeg_blocks(*hdp) * 64;
    if (!coef || cap < need) st = fail(info->message, sizeof info->message, ST_ERR_INVALID, "coef holds %zu values, the stream has %zu", coef ? cap : (size_t)0, need);
  }
  if (st == ST_OK) {
    nseg = st_jpeg_segment_count(*hdp);
    table = new (std::nothrow) uint32_t[2 * nseg];
    if (!table) st = fail(info->message, sizeof info->message, ST_ERR_OOM, "out of host memory for %zu segments", nseg);
  }
  if (st == ST_OK) st = st_jpeg_segments(buf, size, *hdp, table, info->message, sizeof info->message);
  if (st == ST_OK) {
    const StJpegHeader& hd = *hdp;
    size_t most = 1;
    for (size_t k = 0; k < nseg; ++k) most = std::max(most, (size_t)st_jsq_count(table[2 * k + 1] - table[2 * k], (uint32_t)S));
    words = new (std::nothrow) uint64_t[3 * most];
    outs = new (std::nothrow) StJsqOut[most];
    if (!words || !outs) st = fail(info->message, sizeof info->message, ST_ERR_OOM, "out of host memory for %zu subsequences", most);
    memset(tabs, 0, sizeof *tabs);
    for (int c = 0; c < hd.ncomp; ++c) {
      tabs->dc[c] = hd.dc[hd.td[c]];
      tabs->ac[c] = hd.ac[hd.ta[c]];
    }
    const StJpegScanGeom g = st_jpeg_scan_geom(hd);
    const StJpegZigzag zz = st_jpeg_zigzag();
    const long long total = (long long)hd.mcux * hd.mcuy;
    const uint32_t bpm = (uint32_t)st_jsq_mcu_blocks(g);
    if (st == ST_OK) memset(coef, 0, need * sizeof(int16_t));   // the zeroing is a step of its own: two lanes may fill one block
    int most_rounds = 0;
    for (size_t k = 0; k < nseg && st == ST_OK; ++k) {
      const uint32_t begin = table[2 * k], end = table[2 * k + 1];
      const uint32_t nsub = st_jsq_count(end - begin, (uint32_t)S);
      const long long mcu0 = hd.restart_interval > 0 ? (long long)k * hd.restart_interval : 0;
      const long long nmcu = hd.restart_interval > 0 ? std::min<long long>(hd.restart_interval, total - mcu0) : total;
      const uint32_t seg_blocks = (uint32_t)(std::max<long long>(nmcu, 0) * bpm);
      uint64_t *E = words, *En = words + most, *U = words + 2 * most;
      for (uint32_t i = 0; i < nsub; ++i) { E[i] = kStJsqInvalid; U[i] = kStJsqNever; }
      auto sub_end = [&](uint32_t i) { return (uint32_t)std::min<uint64_t>((uint64_t)begin + ((uint64_t)i + 1) * (uint64_t)S, end); };
      bool converged = false;
      int seg_rounds = R;
      for (int r = 1; r <= R && !converged; ++r) {
        bool changed = r == 1;   // the first round gives every lane its first exit
        for (uint32_t i = 0; i < nsub; ++i) {
          const uint64_t enter = i == 0 ? st_jsq_pack(begin, 0, 0, 0) : E[i - 1];
          En[i] = E[i];
          if (enter == U[i]) continue;   // entered from the same state as before: same exit, same counts
          const uint64_t from = enter == kStJsqInvalid ? st_jsq_guess(buf, begin, end, (uint32_t)((uint64_t)begin + (uint64_t)i * (uint64_t)S)) : enter;
          st_jsq_run<false>(buf, end, sub_end(i), false, from, g, tabs, zz.nat, 0, 0, 0, nullptr, nullptr, &outs[i]);
          U[i] = enter;
          En[i] = outs[i].exit;
          changed = changed || En[i] != E[i];
        }
        std::swap(E, En);
        if (!changed) { converged = true; seg_rounds = r - 1; }
        else if ((uint32_t)r >= nsub) { converged = true; seg_rounds = r; }   // lane r - 1 has entered from the true state
      }
      most_rounds = std::max(most_rounds, seg_rounds);
      int je = ST_JE_OK;
      if (!converged) {
        je = st_jpeg_decode_interval(buf, begin, end, mcu0, (int)std::min<long long>(std::max<long long>(nmcu, 0), INT32_MAX), g, tabs, zz.nat, coef);
      } else {
        uint32_t before = 0, dc[3] = {0, 0, 0};
        for (uint32_t i = 0; i < nsub && je == ST_JE_OK && before < seg_blocks; ++i) {
          if (U[i] == kStJsqInvalid) break;   // the chain broke behind the segment's last block
          StJsqOut o;
          je = st_jsq_run<true>(buf, end, sub_end(i), i + 1 == nsub, U[i], g, tabs, zz.nat, mcu0, seg_blocks, before, dc, coef, &o);
          before += o.blocks;
          for (int c = 0; c < 3; ++c) dc[c] = o.dc[c];
        }
      }
      if (je != ST_JE_OK) {
        if (hd.restart_interval > 0)
          st = fail(info->message, sizeof info->message, ST_ERR_INVALID, "corrupt scan: restart interval %zu of %zu: %s", k, nseg, st_jpeg_entropy_cause(je));
        else
          st = fail(info->message, sizeof info->message, ST_ERR_INVALID, "corrupt scan: the scan: %s", st_jpeg_entropy_cause(je));
      }
    }
    if (rounds) *rounds = most_rounds;
    if (st == ST_OK && quant)
      for (int c = 0; c < hd.ncomp; ++c) memcpy(quant + 64 * c, hd.quant[hd.tq[c]], 128);
  }
  delete[] outs;
  delete[] words;
  delete[] table;
  delete tabs;
  delete hdp;
  return st;
}
