// Host side of the ImageEncoder op's PNG output: the refusals, the bound, the exposed code construction and
// st_png_encode_host, the CPU twin of k_png_filter / k_png_deflate / k_png_enc_pack in plain serial C++.  It walks the runs
// where the kernel asks every position for its token, and computes the CRCs and the Adler-32 byte by byte where the kernel
// combines partial ones; the tables come from the shared st_png_enc.h.
#include <cstdio>
#include <cstring>
#include <vector>

#include "scannertools_hip.h"
#include "st_png_enc.h"

#define ST_PNG_EXPORT extern "C" __attribute__((visibility("default")))

extern "C" int st_png_enc_check(int h, int w, int c, int filter, char* msg, size_t msg_len);

namespace {

struct BitWriter {
  std::vector<uint8_t>* out;
  uint64_t acc = 0;
  int n = 0;
  void put(unsigned v, int bits) {
    acc |= (uint64_t)v << n;
    n += bits;
    while (n >= 8) {
      out->push_back((uint8_t)acc);
      acc >>= 8;
      n -= 8;
    }
  }
  void align() {
    if (n) put(0u, 8 - n);
  }
};

uint32_t crc32_bytes(const uint8_t* p, size_t n) {
  struct Table {
    uint32_t v[256];
    Table() { for (uint32_t i = 0; i < 256; ++i) v[i] = st_crc_table_entry(i); }
  };
  static const Table made;
  const uint32_t* table = made.v;
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xffu] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

void put_be32(std::vector<uint8_t>* o, uint32_t v) {
  for (int s = 24; s >= 0; s -= 8) o->push_back((uint8_t)(v >> s));
}

void put_chunk(std::vector<uint8_t>* o, const char* type, const std::vector<uint8_t>& data) {
  put_be32(o, (uint32_t)data.size());
  const size_t at = o->size();
  o->insert(o->end(), type, type + 4);
  o->insert(o->end(), data.begin(), data.end());
  put_be32(o, crc32_bytes(o->data() + at, 4 + data.size()));
}

// the filtered bytes of a frame: per row the type and the row
void filter_frame(const uint8_t* frame, const StPngEncGeom& g, int filter, uint8_t* out) {
  const int rb = g.rb, bpp = g.c;
  for (int y = 0; y < g.h; ++y) {
    const uint8_t* cur = frame + (size_t)y * rb;
    const uint8_t* up = y ? cur - rb : nullptr;
    int ft = filter;
    if (filter == ST_PNG_FILTER_ADAPTIVE) {
      unsigned long long best = ~0ull;
      for (int t = 0; t < 5; ++t) {
        unsigned long long sum = 0;
        for (int i = 0; i < rb; ++i)
          sum += st_png_filter_cost(st_png_filter_byte(t, cur[i], i >= bpp ? cur[i - bpp] : 0, up ? up[i] : 0, up && i >= bpp ? up[i - bpp] : 0));
        if (sum < best) {
          best = sum;
          ft = t;
        }
      }
    }
    uint8_t* o = out + (size_t)y * (1 + rb);
    o[0] = (uint8_t)ft;
    for (int i = 0; i < rb; ++i)
      o[1 + i] = (uint8_t)st_png_filter_byte(ft, cur[i], i >= bpp ? cur[i - bpp] : 0, up ? up[i] : 0, up && i >= bpp ? up[i - bpp] : 0);
  }
}

struct Token { int lit, len; };   // len 0: the literal `lit`

// a piece's deflate data: the dynamic block and the empty stored block, or the piece stored
void deflate_piece(const uint8_t* d, int L, std::vector<uint8_t>* out) {
  std::vector<Token> toks;
  for (int s = 0; s < L;) {
    int e = s + 1;
    while (e < L && d[e] == d[s]) ++e;
    const int R = e - s;
    toks.push_back({d[s], 0});
    int left = R - 1;
    for (; left >= 258; left -= 258) toks.push_back({0, 258});
    if (left >= 3) toks.push_back({0, left});
    else for (; left > 0; --left) toks.push_back({d[s], 0});
    s = e;
  }
  uint32_t freq[kPngLitLen] = {0};
  freq[256] = 1;
  uint64_t extra_bits = 0;
  for (const Token& t : toks) {
    int nb, ex;
    if (t.len) {
      freq[st_png_len_symbol(t.len, &nb, &ex)]++;
      extra_bits += nb + 1;   // and the distance code's one bit
    } else {
      freq[t.lit]++;
    }
  }
  StPngHuffWork wk;
  StPngBlockTables tb;
  const int m = st_png_huff_order(freq, kPngLitLen, &wk);
  st_png_block_tables(&wk, m, &tb);
  uint64_t bits = tb.header_bits + extra_bits;
  for (int i = 0; i < kPngLitLen; ++i) bits += (uint64_t)freq[i] * tb.len[i];
  if (st_png_coded_bytes((uint32_t)bits) >= (uint32_t)(5 + L)) {
    out->push_back(0);
    out->push_back((uint8_t)(L & 0xff));
    out->push_back((uint8_t)(L >> 8));
    out->push_back((uint8_t)(~L & 0xff));
    out->push_back((uint8_t)((~L >> 8) & 0xff));
    out->insert(out->end(), d, d + L);
    return;
  }
  BitWriter bw{out};
  st_png_block_header(tb, [&bw](unsigned v, int n) { bw.put(v, n); });
  for (const Token& t : toks) {
    if (t.len) {
      int nb, ex;
      const int sym = st_png_len_symbol(t.len, &nb, &ex);
      bw.put(tb.code[sym], tb.len[sym]);
      bw.put((unsigned)ex, nb);
      bw.put(0u, 1);   // distance code 0: distance 1
    } else {
      bw.put(tb.code[t.lit], tb.len[t.lit]);
    }
  }
  bw.put(tb.code[256], tb.len[256]);
  bw.put(0u, 3);   // BFINAL = 0, BTYPE = 0
  bw.align();
  for (int v : {0x00, 0x00, 0xFF, 0xFF}) out->push_back((uint8_t)v);
}

}  // namespace

extern "C" int st_png_enc_check(int h, int w, int c, int filter, char* msg, size_t msg_len) {
  msg[0] = 0;
  if (c != 1 && c != 3 && c != 4) {
    snprintf(msg, msg_len, "%d channel(s) cannot be written (1: gray, 3: R, G, B, 4: R, G, B, A)", c);
    return ST_ERR_INVALID;
  }
  if (h < 1 || h > 65535 || w < 1 || w > 65535) {
    snprintf(msg, msg_len, "frame size %dx%d is outside 1..65535", w, h);
    return ST_ERR_INVALID;
  }
  if (filter < ST_PNG_FILTER_NONE || filter > ST_PNG_FILTER_ADAPTIVE) {
    snprintf(msg, msg_len, "filter %d is not supported (ST_PNG_FILTER_NONE = 0 .. ST_PNG_FILTER_PAETH = 4, ST_PNG_FILTER_ADAPTIVE = 5)", filter);
    return ST_ERR_INVALID;
  }
  return ST_OK;
}

ST_PNG_EXPORT int st_png_encode_check(int h, int w, int c, int filter, char* msg, size_t msg_len) {
  char local[160];
  const int st = st_png_enc_check(h, w, c, filter, local, sizeof local);
  if (msg && msg_len) snprintf(msg, msg_len, "%s", local);
  return st;
}

ST_PNG_EXPORT long long st_png_encode_bound(int h, int w, int c) {
  char msg[160];
  if (st_png_enc_check(h, w, c, ST_PNG_FILTER_ADAPTIVE, msg, sizeof msg) != ST_OK) return -1;
  StPngEncGeom g;
  st_png_enc_geom(h, w, c, &g);
  // every piece stored: 12 bytes of chunk and 5 of block header each, the zlib header once
  return (long long)kPngHeadBytes + 2 + (long long)g.fb + 17LL * g.pieces + kPngTailBytes;
}

ST_PNG_EXPORT int st_png_huff_limited(const uint32_t* counts, int symbols, int limit, uint8_t* lengths) {
  if (!counts || !lengths || symbols < 2 || symbols > kPngLitLen || limit < 1 || limit > 15 || (1 << limit) < symbols) return ST_ERR_INVALID;
  uint64_t total = 0;
  for (int i = 0; i < symbols; ++i) total += counts[i];
  if (total >= (1ull << 32)) return ST_ERR_INVALID;
  StPngHuffWork wk;
  const int m = st_png_huff_order(counts, symbols, &wk);
  st_png_huff_lengths(&wk, m, symbols, limit, lengths);
  return ST_OK;
}

ST_PNG_EXPORT int st_png_encode_host(const uint8_t* frame, int h, int w, int c, int filter, uint8_t* buf, size_t cap, size_t* size) {
  char msg[160];
  const int chk = st_png_enc_check(h, w, c, filter, msg, sizeof msg);
  if (chk != ST_OK) return chk;
  if (!frame || !size) return ST_ERR_INVALID;
  StPngEncGeom g;
  st_png_enc_geom(h, w, c, &g);
  std::vector<uint8_t> raw(g.fb), out, data;
  filter_frame(frame, g, filter, raw.data());
  out.reserve((size_t)st_png_encode_bound(h, w, c));
  for (int v : {0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A}) out.push_back((uint8_t)v);
  put_be32(&data, (uint32_t)w);
  put_be32(&data, (uint32_t)h);
  for (int v : {8, c == 1 ? 0 : c == 3 ? 2 : 6, 0, 0, 0}) data.push_back((uint8_t)v);
  put_chunk(&out, "IHDR", data);
  uint32_t a = 1, b = 0;
  for (int p = 0; p < g.pieces; ++p) {
    const uint8_t* d = raw.data() + (size_t)p * kPngPiece;
    const int L = st_png_piece_len(g.fb, p);
    data.clear();
    if (p == 0) {
      data.push_back(0x78);
      data.push_back(0x01);
    }
    deflate_piece(d, L, &data);
    put_chunk(&out, "IDAT", data);
    for (int i = 0; i < L; ++i) {
      a = (a + d[i]) % kAdlerMod;
      b = (b + a) % kAdlerMod;
    }
  }
  data.clear();
  for (int v : {0x01, 0x00, 0x00, 0xFF, 0xFF}) data.push_back((uint8_t)v);
  put_be32(&data, b << 16 | a);
  put_chunk(&out, "IDAT", data);
  data.clear();
  put_chunk(&out, "IEND", data);
  *size = out.size();
  if (!buf) return ST_OK;   // the size alone
  if (cap < out.size()) return ST_ERR_INVALID;
  memcpy(buf, out.data(), out.size());
  return ST_OK;
}
