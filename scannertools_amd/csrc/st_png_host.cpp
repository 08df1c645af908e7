// PNG on the host: container parser (chunk framing, CRC-32, IHDR / PLTE / tRNS / IDAT order), the library's own zlib-stream
// inflater (RFC 1950 / 1951: stored, fixed and dynamic blocks, Adler-32) and the CPU twin of the kernels of st_png.hip.
// No device code and no HIP header: this file also compiles with a plain C++ compiler (scripts/png_host_check.cpp).
#include "st_png_host.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>

#define ST_PNG_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

int fail(char* msg, size_t msg_len, int status, const char* fmt, ...) {
  if (msg && msg_len) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, msg_len, fmt, ap);
    va_end(ap);
  }
  return status;
}

// ---- CRC-32 (PNG annex D) and Adler-32 ---------------------------------------------------------------------------------------
struct CrcTable {   // slicing by 8: t[k][b] is the CRC of byte b followed by k zero bytes
  uint32_t t[8][256];
  constexpr CrcTable() : t() {
    for (uint32_t n = 0; n < 256; ++n) {
      uint32_t c = n;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xedb88320u ^ (c >> 1) : c >> 1;
      t[0][n] = c;
    }
    for (uint32_t n = 0; n < 256; ++n)
      for (int k = 1; k < 8; ++k) t[k][n] = t[0][t[k - 1][n] & 0xff] ^ (t[k - 1][n] >> 8);
  }
};
constexpr CrcTable kCrc;

uint32_t crc32(const uint8_t* p, size_t n) {
  uint32_t c = 0xffffffffu;
  for (; n >= 8; p += 8, n -= 8) {
    uint32_t lo, hi;   // little-endian host
    memcpy(&lo, p, 4);
    memcpy(&hi, p + 4, 4);
    lo ^= c;
    c = kCrc.t[7][lo & 0xff] ^ kCrc.t[6][(lo >> 8) & 0xff] ^ kCrc.t[5][(lo >> 16) & 0xff] ^ kCrc.t[4][lo >> 24] ^
        kCrc.t[3][hi & 0xff] ^ kCrc.t[2][(hi >> 8) & 0xff] ^ kCrc.t[1][(hi >> 16) & 0xff] ^ kCrc.t[0][hi >> 24];
  }
  for (size_t i = 0; i < n; ++i) c = kCrc.t[0][(c ^ p[i]) & 0xff] ^ (c >> 8);
  return c ^ 0xffffffffu;
}

uint32_t adler32(const uint8_t* p, size_t n) {
  uint32_t a = 1, b = 0;
  while (n) {
    const size_t k = n < 5552 ? n : 5552;   // the most bytes before b can pass 2^32
    for (size_t i = 0; i < k; ++i) { a += p[i]; b += a; }
    a %= 65521u;
    b %= 65521u;
    p += k;
    n -= k;
  }
  return b << 16 | a;
}

inline uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// ---- the inflater ------------------------------------------------------------------------------------------------------------
// Bits come LSB first from the joined pieces.  Past the end of the input zero bytes are fed and counted (`fake` bits); the
// stream is truncated as soon as a consumed bit was one of them.
struct BitIn {
  const uint8_t* base;
  const StPngIdat* pieces;
  size_t npieces, piece;
  const uint8_t *p, *end;
  uint64_t bits;
  int nbits, fake;

  void next_piece() {
    while (p == end && piece + 1 < npieces) {
      ++piece;
      p = base + pieces[piece].off;
      end = p + pieces[piece].len;
    }
  }
  void refill() {
    if (nbits > 56) return;
    if (end - p >= 8) {
      uint64_t v;
      memcpy(&v, p, 8);   // little-endian host (x86-64, as the rest of the library assumes)
      bits |= v << nbits;
      const int adv = (63 - nbits) >> 3;
      p += adv;
      nbits += adv * 8;
      bits &= ((uint64_t)1 << nbits) - 1;
      return;
    }
    while (nbits <= 56) {
      if (p == end) next_piece();
      if (p == end) { nbits += 8; fake += 8; continue; }
      bits |= (uint64_t)*p++ << nbits;
      nbits += 8;
    }
  }
  uint32_t peek(int n) const { return (uint32_t)(bits & (((uint64_t)1 << n) - 1)); }
  void drop(int n) { bits >>= n; nbits -= n; }
  uint32_t take(int n) { const uint32_t v = peek(n); drop(n); return v; }
  bool truncated() const { return nbits < fake; }
};

constexpr int kFastBits = 10;
struct Huff {
  uint16_t count[16];       // codes of each length
  uint16_t symbol[288];     // symbols in canonical order
  uint16_t fast[1 << kFastBits];   // by the next kFastBits bits: symbol << 4 | length; 0: longer than kFastBits, or no such code
};

// 0: a complete code; 1: over-subscribed; 2: incomplete.  `ones`: the set is one code of length 1; `none`: no code at all.
int build_huff(const uint8_t* lens, int n, Huff* h, bool* ones, bool* none) {
  memset(h->count, 0, sizeof h->count);
  for (int i = 0; i < n; ++i) h->count[lens[i]]++;
  *none = h->count[0] == n;
  *ones = h->count[1] == 1 && h->count[0] == n - 1;
  int left = 1;
  for (int l = 1; l <= 15; ++l) {
    left <<= 1;
    left -= h->count[l];
    if (left < 0) return 1;
  }
  uint16_t offs[16];
  offs[1] = 0;
  for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + h->count[l]);
  for (int i = 0; i < n; ++i)
    if (lens[i]) h->symbol[offs[lens[i]]++] = (uint16_t)i;
  memset(h->fast, 0, sizeof h->fast);
  // canonical codes, bit-reversed (the stream holds a code's first bit lowest), replicated over the unused high bits
  int code = 0, idx = 0;
  for (int l = 1; l <= kFastBits; ++l) {
    for (int k = 0; k < h->count[l]; ++k, ++code, ++idx) {
      int rev = 0;
      for (int b = 0; b < l; ++b) rev |= ((code >> b) & 1) << (l - 1 - b);
      for (int f = rev; f < (1 << kFastBits); f += 1 << l) h->fast[f] = (uint16_t)(h->symbol[idx] << 4 | l);
    }
    code <<= 1;
  }
  h->count[0] = 0;
  return left > 0 ? 2 : 0;
}

// the next symbol; -1: no such code (an incomplete set).  Needs 15 bits in the buffer.
inline int decode_sym(BitIn& in, const Huff& h) {
  const uint16_t e = h.fast[in.peek(kFastBits)];
  if (e) {
    in.drop(e & 15);
    return e >> 4;
  }
  int code = 0, first = 0, index = 0;
  uint32_t v = in.peek(15);
  for (int l = 1; l <= 15; ++l) {
    code |= (int)(v & 1);
    v >>= 1;
    const int count = h.count[l];
    if (code - count < first) {
      in.drop(l);
      return h.symbol[index + (code - first)];
    }
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

const uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
const uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
const uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
const uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

#define INF_FAIL(...) return fail(msg, msg_len, ST_ERR_INVALID, __VA_ARGS__)

int inflate_impl(const uint8_t* base, const StPngIdat* pieces, size_t npieces, uint8_t* dst, size_t cap, size_t* produced, char* msg,
                 size_t msg_len) {
  if (msg && msg_len) msg[0] = 0;
  if (produced) *produced = 0;
  static const StPngIdat kNone = {0, 0};
  BitIn in;
  in.base = base;
  in.pieces = npieces ? pieces : &kNone;
  in.npieces = npieces ? npieces : 1;
  in.piece = 0;
  in.p = base + in.pieces[0].off;
  in.end = in.p + in.pieces[0].len;
  in.bits = 0;
  in.nbits = 0;
  in.fake = 0;
  in.refill();
  const uint32_t cmf = in.take(8), flg = in.take(8);
  if (in.truncated()) INF_FAIL("zlib: truncated input (no header)");
  if ((cmf & 15) != 8) INF_FAIL("zlib: compression method %u is not deflate (8)", cmf & 15);
  if ((cmf >> 4) > 7) INF_FAIL("zlib: window of 2^%u bytes exceeds 32 KiB", (cmf >> 4) + 8);
  if ((cmf << 8 | flg) % 31) INF_FAIL("zlib: header check (FCHECK) fails");
  if (flg & 0x20) INF_FAIL("zlib: a preset dictionary is not supported");
  size_t out = 0;
  Huff lit, dist;
  uint8_t lens[320];
  for (bool last = false; !last;) {
    in.refill();
    last = in.take(1) != 0;
    const uint32_t type = in.take(2);
    if (in.truncated()) INF_FAIL("inflate: truncated input (block header)");
    if (type == 3) INF_FAIL("inflate: block type 3 is reserved");
    if (type == 0) {
      in.drop(in.nbits & 7);
      in.refill();
      const uint32_t len = in.take(16), nlen = in.take(16);
      if (in.truncated()) INF_FAIL("inflate: truncated input (stored block header)");
      if ((len ^ 0xffffu) != nlen) INF_FAIL("inflate: stored block LEN/NLEN mismatch (%04x / %04x)", len, nlen);
      if (len > cap - out) INF_FAIL("inflate: more output than the buffer holds (%zu bytes)", cap);
      uint32_t left = len;
      // what the bit buffer already holds, then straight from the pieces
      while (left && in.nbits > in.fake) { dst[out++] = (uint8_t)in.take(8); --left; }
      if (left) { in.bits = 0; in.nbits = 0; in.fake = 0; }
      while (left) {
        if (in.p == in.end) in.next_piece();
        if (in.p == in.end) INF_FAIL("inflate: truncated input (stored block of %u bytes)", len);
        const size_t k = (size_t)(in.end - in.p) < left ? (size_t)(in.end - in.p) : left;
        memcpy(dst + out, in.p, k);
        in.p += k;
        out += k;
        left -= (uint32_t)k;
      }
      continue;
    }
    bool ones, none, dist_none = false;
    if (type == 1) {
      for (int i = 0; i < 144; ++i) lens[i] = 8;
      for (int i = 144; i < 256; ++i) lens[i] = 9;
      for (int i = 256; i < 280; ++i) lens[i] = 7;
      for (int i = 280; i < 288; ++i) lens[i] = 8;
      build_huff(lens, 288, &lit, &ones, &none);
      for (int i = 0; i < 32; ++i) lens[i] = 5;
      build_huff(lens, 32, &dist, &ones, &none);
    } else {
      in.refill();
      const int hlit = (int)in.take(5) + 257, hdist = (int)in.take(5) + 1, hclen = (int)in.take(4) + 4;
      if (in.truncated()) INF_FAIL("inflate: truncated input (dynamic block header)");
      if (hlit > 286 || hdist > 30) INF_FAIL("inflate: too many length or distance symbols (%d / %d)", hlit, hdist);
      uint8_t cl[19];
      memset(cl, 0, sizeof cl);
      for (int i = 0; i < hclen; ++i) {
        in.refill();
        cl[kClOrder[i]] = (uint8_t)in.take(3);
      }
      if (in.truncated()) INF_FAIL("inflate: truncated input (code length codes)");
      Huff clh;
      int r = build_huff(cl, 19, &clh, &ones, &none);
      if (r == 1) INF_FAIL("inflate: over-subscribed code length code set");
      if (r == 2) INF_FAIL("inflate: incomplete code length code set");
      int i = 0;
      while (i < hlit + hdist) {
        in.refill();
        const int s = decode_sym(in, clh);
        if (in.truncated()) INF_FAIL("inflate: truncated input (code lengths)");
        if (s < 0) INF_FAIL("inflate: invalid code in the code lengths");
        if (s < 16) { lens[i++] = (uint8_t)s; continue; }
        int rep, val = 0;
        if (s == 16) {
          if (i == 0) INF_FAIL("inflate: code length repeat with no previous length");
          val = lens[i - 1];
          rep = 3 + (int)in.take(2);
        } else if (s == 17) rep = 3 + (int)in.take(3);
        else rep = 11 + (int)in.take(7);
        if (in.truncated()) INF_FAIL("inflate: truncated input (code lengths)");
        if (i + rep > hlit + hdist) INF_FAIL("inflate: code length repeat runs past the %d lengths", hlit + hdist);
        while (rep--) lens[i++] = (uint8_t)val;
      }
      if (lens[256] == 0) INF_FAIL("inflate: incomplete literal/length code set (no end-of-block code)");
      r = build_huff(lens, hlit, &lit, &ones, &none);
      if (r == 1) INF_FAIL("inflate: over-subscribed literal/length code set");
      if (r == 2 && !ones) INF_FAIL("inflate: incomplete literal/length code set");
      r = build_huff(lens + hlit, hdist, &dist, &ones, &none);
      if (r == 1) INF_FAIL("inflate: over-subscribed distance code set");
      if (r == 2 && !ones && !none) INF_FAIL("inflate: incomplete distance code set");
      dist_none = none;
    }
    for (;;) {
      in.refill();
      int s = decode_sym(in, lit);
      if (in.truncated()) INF_FAIL("inflate: truncated input after %zu bytes of output", out);
      if (s < 0) INF_FAIL("inflate: invalid literal/length code");
      if (s < 256) {
        if (out >= cap) INF_FAIL("inflate: more output than the buffer holds (%zu bytes)", cap);
        dst[out++] = (uint8_t)s;
        continue;
      }
      if (s == 256) break;
      s -= 257;
      if (s >= 29) INF_FAIL("inflate: invalid length symbol %d", s + 257);
      const size_t len = kLenBase[s] + in.take(kLenExtra[s]);
      if (dist_none) INF_FAIL("inflate: a distance code in a block that declares none");
      const int d = decode_sym(in, dist);
      if (d < 0) INF_FAIL("inflate: invalid distance code");
      if (d >= 30) INF_FAIL("inflate: invalid distance symbol %d", d);
      const size_t back = kDistBase[d] + in.take(kDistExtra[d]);
      if (in.truncated()) INF_FAIL("inflate: truncated input after %zu bytes of output", out);
      if (back > out) INF_FAIL("inflate: distance %zu reaches before the start of the output (%zu bytes so far)", back, out);
      if (len > cap - out) INF_FAIL("inflate: more output than the buffer holds (%zu bytes)", cap);
      const uint8_t* from = dst + out - back;
      uint8_t* to = dst + out;
      if (back >= len) memcpy(to, from, len);
      else for (size_t k = 0; k < len; ++k) to[k] = from[k];
      out += len;
    }
  }
  in.drop(in.nbits & 7);
  in.refill();
  const uint32_t want = in.take(8) << 24 | in.take(8) << 16 | in.take(8) << 8 | in.take(8);
  if (in.truncated()) INF_FAIL("zlib: truncated input (no Adler-32 trailer)");
  const uint32_t got = adler32(dst, out);
  if (got != want) INF_FAIL("zlib: Adler-32 mismatch (stream %08x, data %08x)", want, got);
  if (produced) *produced = out;
  return ST_OK;
}

// ---- the container -------------------------------------------------------------------------------------------------------------
#define PNG_FAIL(status, ...) return fail(msg, msg_len, status, __VA_ARGS__)

inline uint32_t fourcc(const char* s) { return (uint32_t)(uint8_t)s[0] << 24 | (uint32_t)(uint8_t)s[1] << 16 | (uint32_t)(uint8_t)s[2] << 8 | (uint8_t)s[3]; }

int paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

}  // namespace

int st_zlib_inflate_pieces(const uint8_t* base, const StPngIdat* pieces, size_t npieces, uint8_t* dst, size_t cap, size_t* produced,
                           char* msg, size_t msg_len) {
  return inflate_impl(base, pieces, npieces, dst, cap, produced, msg, msg_len);
}

static int st_png_check_idat_crcs(const uint8_t* buf, const StPngHeader& hd, char* msg, size_t msg_len) {
  for (const StPngIdat& c : hd.idat)
    if (crc32(buf + c.off - 4, c.len + 4) != be32(buf + c.off + c.len)) return fail(msg, msg_len, ST_ERR_INVALID, "png: chunk IDAT fails its CRC-32");
  return ST_OK;
}

int st_png_parse(const uint8_t* buf, size_t size, bool full, StPngHeader* hd, char* msg, size_t msg_len) {
  static const uint8_t kSig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  if (msg && msg_len) msg[0] = 0;
  hd->h = hd->w = hd->channels = hd->color_type = hd->bit_depth = hd->interlace = 0;
  hd->npal = hd->ntrns = hd->has_trns = hd->bpp = hd->rowbytes = hd->kind = 0;
  hd->idat.clear();
  hd->idat_bytes = 0;
  memset(hd->key, 0, sizeof hd->key);
  for (int i = 0; i < 256; ++i) { hd->pal[4 * i] = hd->pal[4 * i + 1] = hd->pal[4 * i + 2] = 0; hd->pal[4 * i + 3] = 255; }
  if (!buf) PNG_FAIL(ST_ERR_INVALID, "png: null stream");
  if (size < 8 || memcmp(buf, kSig, 8) != 0) PNG_FAIL(ST_ERR_INVALID, "png: not a PNG stream (bad signature)");
  size_t pos = 8;
  bool have_ihdr = false, have_plte = false, in_idat = false, idat_done = false;
  for (;;) {
    if (size - pos < 12) PNG_FAIL(ST_ERR_INVALID, "png: truncated stream: %s", !have_ihdr ? "no IHDR chunk" : (hd->idat_bytes || in_idat ? "no IEND chunk" : "no IDAT chunk"));
    const uint32_t len = be32(buf + pos), type = be32(buf + pos + 4);
    char name[5] = {(char)buf[pos + 4], (char)buf[pos + 5], (char)buf[pos + 6], (char)buf[pos + 7], 0};
    for (int k = 0; k < 4; ++k)
      if (!((name[k] >= 'A' && name[k] <= 'Z') || (name[k] >= 'a' && name[k] <= 'z'))) PNG_FAIL(ST_ERR_INVALID, "png: invalid chunk type at byte %zu", pos + 4);
    if (len > 0x7fffffffu || (size_t)len > size - pos - 12) PNG_FAIL(ST_ERR_INVALID, "png: truncated stream: chunk %s of %u bytes runs past the end", name, len);
    const uint8_t* data = buf + pos + 8;
    // (the IDAT chunks hold nearly all of a stream's bytes: their CRCs are checked with the data, st_png_inflate_rows)
    const bool checked = type == fourcc("IHDR") || type == fourcc("PLTE") || type == fourcc("tRNS") || type == fourcc("IEND");
    if (checked && crc32(buf + pos + 4, (size_t)len + 4) != be32(data + len)) PNG_FAIL(ST_ERR_INVALID, "png: chunk %s fails its CRC-32", name);
    if (!have_ihdr && type != fourcc("IHDR")) PNG_FAIL(ST_ERR_INVALID, "png: the first chunk is %s, not IHDR", name);
    if (in_idat && type != fourcc("IDAT")) { in_idat = false; idat_done = true; }
    if (type == fourcc("IHDR")) {
      if (have_ihdr) PNG_FAIL(ST_ERR_INVALID, "png: a second IHDR chunk");
      if (len != 13) PNG_FAIL(ST_ERR_INVALID, "png: IHDR of %u bytes, not 13", len);
      have_ihdr = true;
      const uint32_t w = be32(data), h = be32(data + 4);
      const int depth = data[8], ct = data[9];
      if (w == 0 || h == 0 || w > 0x7fffffffu || h > 0x7fffffffu) PNG_FAIL(ST_ERR_INVALID, "png: invalid size %ux%u", w, h);
      const bool depth_ok = ct == 0 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16)
                          : ct == 3 ? (depth == 1 || depth == 2 || depth == 4 || depth == 8)
                          : (ct == 2 || ct == 4 || ct == 6) ? (depth == 8 || depth == 16) : false;
      if (!depth_ok) PNG_FAIL(ST_ERR_INVALID, "png: invalid colour type %d / bit depth %d", ct, depth);
      if (data[10] != 0) PNG_FAIL(ST_ERR_INVALID, "png: invalid compression method %d", data[10]);
      if (data[11] != 0) PNG_FAIL(ST_ERR_INVALID, "png: invalid filter method %d", data[11]);
      if (data[12] > 1) PNG_FAIL(ST_ERR_INVALID, "png: invalid interlace method %d", data[12]);
      hd->color_type = ct;
      hd->bit_depth = depth;
      hd->interlace = data[12];
      if (depth == 16) PNG_FAIL(ST_ERR_UNSUPPORTED, "png: 16-bit samples are not supported");
      if (data[12] == 1) PNG_FAIL(ST_ERR_UNSUPPORTED, "png: Adam7 interlace is not supported");
      if (w > 65535 || h > 65535) PNG_FAIL(ST_ERR_UNSUPPORTED, "png: %ux%u is larger than 65535 in a dimension", w, h);
      hd->w = (int)w;
      hd->h = (int)h;
      const int samples = ct == 0 || ct == 3 ? 1 : ct == 4 ? 2 : ct == 2 ? 3 : 4;
      hd->rowbytes = (int)(((size_t)w * samples * depth + 7) / 8);
      hd->bpp = depth < 8 ? 1 : samples;
      if ((size_t)h * (1 + (size_t)hd->rowbytes) >= ((size_t)2 << 30)) PNG_FAIL(ST_ERR_UNSUPPORTED, "png: %ux%u needs 2 GiB or more of scanlines", w, h);
      hd->channels = ct == 0 ? 1 : ct == 2 || ct == 3 ? 3 : 4;
      hd->kind = ct == 0 ? (depth < 8 ? ST_PNG_GRAY_BITS : ST_PNG_DIRECT) : ct == 3 ? ST_PNG_PALETTE : ct == 4 ? ST_PNG_GRAY_ALPHA : ST_PNG_DIRECT;
    } else if (type == fourcc("PLTE")) {
      if (have_plte) PNG_FAIL(ST_ERR_INVALID, "png: a second PLTE chunk");
      if (in_idat || idat_done || hd->idat_bytes) PNG_FAIL(ST_ERR_INVALID, "png: PLTE after IDAT");
      if (hd->has_trns) PNG_FAIL(ST_ERR_INVALID, "png: PLTE after tRNS");
      if (hd->color_type == 0 || hd->color_type == 4) PNG_FAIL(ST_ERR_INVALID, "png: PLTE in a gray image");
      if (len == 0 || len % 3 || len > 768) PNG_FAIL(ST_ERR_INVALID, "png: PLTE of %u bytes", len);
      have_plte = true;
      hd->npal = (int)(len / 3);
      if (hd->color_type == 3)
        for (int i = 0; i < hd->npal; ++i) { hd->pal[4 * i] = data[3 * i]; hd->pal[4 * i + 1] = data[3 * i + 1]; hd->pal[4 * i + 2] = data[3 * i + 2]; }
    } else if (type == fourcc("tRNS")) {
      if (hd->has_trns) PNG_FAIL(ST_ERR_INVALID, "png: a second tRNS chunk");
      if (in_idat || idat_done || hd->idat_bytes) PNG_FAIL(ST_ERR_INVALID, "png: tRNS after IDAT");
      const int ct = hd->color_type;
      if (ct == 4 || ct == 6) PNG_FAIL(ST_ERR_INVALID, "png: tRNS in an image with an alpha channel");
      if (ct == 3 && !have_plte) PNG_FAIL(ST_ERR_INVALID, "png: tRNS before PLTE");
      if ((ct == 0 && len != 2) || (ct == 2 && len != 6) || (ct == 3 && (len == 0 || (int)len > hd->npal)))
        PNG_FAIL(ST_ERR_INVALID, "png: tRNS of %u bytes for colour type %d", len, ct);
      hd->has_trns = 1;
      hd->ntrns = (int)len;
      if (ct == 2) {
        hd->key[0] = data[1]; hd->key[1] = data[3]; hd->key[2] = data[5];   // 16-bit values; at depth 8 the low bytes
        hd->kind = ST_PNG_RGB_KEY;
        hd->channels = 4;
      } else if (ct == 3) {
        for (uint32_t i = 0; i < len; ++i) hd->pal[4 * i + 3] = data[i];
        hd->channels = 4;
      }
    } else if (type == fourcc("IDAT")) {
      if (idat_done) PNG_FAIL(ST_ERR_INVALID, "png: IDAT chunks are not consecutive");
      if (hd->color_type == 3 && !have_plte) PNG_FAIL(ST_ERR_INVALID, "png: a palette image without PLTE before IDAT");
      if (!full) return ST_OK;
      in_idat = true;
      hd->idat.push_back(StPngIdat{(size_t)(data - buf), (size_t)len});
      hd->idat_bytes += len;
    } else if (type == fourcc("IEND")) {
      if (len != 0) PNG_FAIL(ST_ERR_INVALID, "png: IEND of %u bytes", len);
      if (hd->idat.empty()) PNG_FAIL(ST_ERR_INVALID, "png: no IDAT chunk");
      return ST_OK;
    } else if (!(name[0] & 0x20)) {
      PNG_FAIL(ST_ERR_INVALID, "png: unknown critical chunk %s", name);
    }
    pos += 12 + (size_t)len;
  }
}

void st_png_fill_info(const StPngHeader& hd, st_png_info* info) {
  info->h = hd.h; info->w = hd.w; info->channels = hd.channels;
  info->color_type = hd.color_type; info->bit_depth = hd.bit_depth; info->interlace = hd.interlace;
  info->palette_entries = hd.npal; info->trns_entries = hd.ntrns;
}

int st_png_inflate_rows(const uint8_t* buf, const StPngHeader& hd, uint8_t* raw, char* msg, size_t msg_len) {
  const size_t need = st_png_raw_bytes(hd);
  size_t got = 0;
  const int crc = st_png_check_idat_crcs(buf, hd, msg, msg_len);
  if (crc != ST_OK) return crc;
  char m[128];
  const int st = st_zlib_inflate_pieces(buf, hd.idat.data(), hd.idat.size(), raw, need, &got, m, sizeof m);
  if (st != ST_OK) return fail(msg, msg_len, st, "png: %s", m);
  if (got != need) return fail(msg, msg_len, ST_ERR_INVALID, "png: inflated length %zu, a %dx%d image needs exactly %zu", got, hd.w, hd.h, need);
  for (int y = 0; y < hd.h; ++y) {
    const int ft = raw[(size_t)y * (1 + (size_t)hd.rowbytes)];
    if (ft > 4) return fail(msg, msg_len, ST_ERR_INVALID, "png: row %d has filter type %d", y, ft);
  }
  return ST_OK;
}

void st_png_unfilter_host(const StPngHeader& hd, const uint8_t* raw, uint8_t* recon) {
  const int rb = hd.rowbytes, bpp = hd.bpp;
  for (int y = 0; y < hd.h; ++y) {
    const uint8_t* x = raw + (size_t)y * (1 + (size_t)rb);
    const int ft = *x++;
    uint8_t* o = recon + (size_t)y * rb;
    const uint8_t* up = y ? o - rb : nullptr;
    for (int i = 0; i < rb; ++i) {
      const int a = i >= bpp ? o[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= bpp) ? up[i - bpp] : 0;
      const int pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ft == 4 ? paeth(a, b, c) : 0;
      o[i] = (uint8_t)(x[i] + pred);
    }
  }
}

void st_png_expand_host(const StPngHeader& hd, const uint8_t* recon, uint8_t* frame) {
  const int rb = hd.rowbytes, w = hd.w, ch = hd.channels, depth = hd.bit_depth;
  const int scale = depth == 1 ? 255 : depth == 2 ? 85 : depth == 4 ? 17 : 1;
  for (int y = 0; y < hd.h; ++y) {
    const uint8_t* r = recon + (size_t)y * rb;
    uint8_t* o = frame + (size_t)y * w * ch;
    for (int x = 0; x < w; ++x) {
      switch (hd.kind) {
        case ST_PNG_DIRECT:
          for (int k = 0; k < ch; ++k) o[x * ch + k] = r[x * ch + k];
          break;
        case ST_PNG_GRAY_BITS:
        case ST_PNG_PALETTE: {
          const int bit = x * depth;   // samples are packed from the most significant bit down
          const int v = depth == 8 ? r[x] : (r[bit >> 3] >> (8 - depth - (bit & 7))) & ((1 << depth) - 1);
          if (hd.kind == ST_PNG_GRAY_BITS) o[x] = (uint8_t)(v * scale);
          else for (int k = 0; k < ch; ++k) o[x * ch + k] = hd.pal[4 * v + k];
          break;
        }
        case ST_PNG_GRAY_ALPHA:
          o[4 * x] = o[4 * x + 1] = o[4 * x + 2] = r[2 * x];
          o[4 * x + 3] = r[2 * x + 1];
          break;
        case ST_PNG_RGB_KEY: {
          const uint8_t R = r[3 * x], G = r[3 * x + 1], B = r[3 * x + 2];
          o[4 * x] = R; o[4 * x + 1] = G; o[4 * x + 2] = B;
          o[4 * x + 3] = (R == hd.key[0] && G == hd.key[1] && B == hd.key[2]) ? 0 : 255;
          break;
        }
      }
    }
  }
}

// ---- C ABI (host only) ----------------------------------------------------------------------------------------------------
ST_PNG_EXPORT int st_png_probe(const uint8_t* buf, size_t size, st_png_info* info) {
  if (!info) return ST_ERR_INVALID;
  memset(info, 0, sizeof *info);
  StPngHeader hd;
  const int st = st_png_parse(buf, size, false, &hd, info->message, sizeof info->message);
  st_png_fill_info(hd, info);
  return st;
}

ST_PNG_EXPORT int st_zlib_inflate(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* produced, char* message, size_t message_len) {
  if (!src || (!dst && cap)) return fail(message, message_len, ST_ERR_INVALID, "zlib: null argument");
  const StPngIdat piece = {0, n};
  return st_zlib_inflate_pieces(src, &piece, 1, dst, cap, produced, message, message_len);
}

ST_PNG_EXPORT int st_png_filtered(const uint8_t* buf, size_t size, uint8_t* raw, size_t cap, st_png_info* info) {
  if (!info) return ST_ERR_INVALID;
  memset(info, 0, sizeof *info);
  StPngHeader hd;
  const int st = st_png_parse(buf, size, true, &hd, info->message, sizeof info->message);
  st_png_fill_info(hd, info);
  if (st != ST_OK) return st;
  if (!raw || cap < st_png_raw_bytes(hd))
    return fail(info->message, sizeof info->message, ST_ERR_INVALID, "png: the scanlines need %zu bytes, the buffer has %zu", st_png_raw_bytes(hd), raw ? cap : (size_t)0);
  return st_png_inflate_rows(buf, hd, raw, info->message, sizeof info->message);
}

ST_PNG_EXPORT int st_png_decode_host(const uint8_t* buf, size_t size, uint8_t* frame, size_t cap, st_png_info* info) {
  if (!info) return ST_ERR_INVALID;
  memset(info, 0, sizeof *info);
  StPngHeader hd;
  const int st = st_png_parse(buf, size, true, &hd, info->message, sizeof info->message);
  st_png_fill_info(hd, info);
  if (st != ST_OK) return st;
  if (!frame || cap < st_png_frame_bytes(hd))
    return fail(info->message, sizeof info->message, ST_ERR_INVALID, "png: the frame needs %zu bytes, the buffer has %zu", st_png_frame_bytes(hd), frame ? cap : (size_t)0);
  std::vector<uint8_t> raw, recon;
  try {
    raw.resize(st_png_raw_bytes(hd));
    recon.resize((size_t)hd.h * hd.rowbytes);
  } catch (...) {
    return fail(info->message, sizeof info->message, ST_ERR_OOM, "png: out of host memory");
  }
  const int s2 = st_png_inflate_rows(buf, hd, raw.data(), info->message, sizeof info->message);
  if (s2 != ST_OK) return s2;
  st_png_unfilter_host(hd, raw.data(), recon.data());
  st_png_expand_host(hd, recon.data(), frame);
  return ST_OK;
}
