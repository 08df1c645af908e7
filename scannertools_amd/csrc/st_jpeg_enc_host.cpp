// Host side of the ImageEncoder op (see st_jpeg_enc_host.h): st_jpeg_quant_tables, st_jpeg_encode_header(_rst),
// st_jpeg_encode_bound and what st_jpeg_enc.hip shares with them.  The tables are those of ITU-T T.81 Annex K; the scaling is
// libjpeg's jpeg_set_quality with force_baseline; the marker order is libjpeg's.
#include "st_jpeg_enc_host.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "scannertools_hip.h"
#include "st_jpeg_enc_opt.h"

#define ST_JPEG_EXPORT extern "C" __attribute__((visibility("default")))

const uint8_t st_jpeg_enc_zigzag[64] = {ST_JPEG_ENC_ZIGZAG};

namespace {

// T.81 tables K.1 and K.2, natural order
const uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                               69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                               81, 104, 113, 92, 49, 64, 78, 87,  103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                 99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// T.81 tables K.3 - K.6: codes per length 1 .. 16, then the symbols in code order
const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

struct HuffSpec { const uint8_t* bits; const uint8_t* vals; int nvals; int cls_id; int tab_off; };
const HuffSpec kHuff[4] = {{kDcLumaBits, kDcVals, 12, 0x00, 0},         // in the order libjpeg writes the DHT segments
                           {kAcLumaBits, kAcLumaVals, 162, 0x10, 32},
                           {kDcChromaBits, kDcVals, 12, 0x01, 16},
                           {kAcChromaBits, kAcChromaVals, 162, 0x11, 288}};

bool sampling_ok(int hs, int vs) { return (hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2); }

}  // namespace

int st_jpeg_enc_check(int h, int w, int quality, int h_samp, int v_samp, char* msg, size_t msg_len) {
  msg[0] = 0;
  if (quality < 1 || quality > 100) {
    snprintf(msg, msg_len, "quality %d is outside 1..100", quality);
    return ST_ERR_INVALID;
  }
  if (!sampling_ok(h_samp, v_samp)) {
    snprintf(msg, msg_len, "luma sampling %dx%d is not supported (1x1, 2x1 or 2x2)", h_samp, v_samp);
    return ST_ERR_UNSUPPORTED;
  }
  if (h < 1 || h > 65535 || w < 1 || w > 65535) {
    snprintf(msg, msg_len, "frame size %dx%d is outside 1..65535", w, h);
    return ST_ERR_INVALID;
  }
  return ST_OK;
}

int st_jpeg_enc_check_restart(int restart, char* msg, size_t msg_len) {
  msg[0] = 0;
  if (restart != ST_JPEG_RESTART_ROW && restart != ST_JPEG_RESTART_NONE) {
    snprintf(msg, msg_len, "restart %d is not supported (ST_JPEG_RESTART_ROW = 0 or ST_JPEG_RESTART_NONE = 1)", restart);
    return ST_ERR_INVALID;
  }
  return ST_OK;
}

void st_jpeg_enc_geom(int h, int w, int hs, int vs, StJpegEncGeom* g) {
  g->h = h; g->w = w; g->hs = hs; g->vs = vs;
  g->mcols = (w + 8 * hs - 1) / (8 * hs);
  g->mrows = (h + 8 * vs - 1) / (8 * vs);
  g->bpm = hs * vs + 2;
  g->nbx = (w + 7) / 8;
  g->nby = (h + 7) / 8;
  g->cw = (w + hs - 1) / hs;
  g->ch = (h + vs - 1) / vs;
}

void st_jpeg_enc_huff(uint32_t* tab) {
  memset(tab, 0, sizeof(uint32_t) * kJpegEncHuffWords);
  for (const HuffSpec& s : kHuff) {
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < s.bits[len - 1]; ++i) tab[s.tab_off + s.vals[k++]] = ((uint32_t)len << 16) | code++;
      code <<= 1;
    }
  }
}

ST_JPEG_EXPORT int st_jpeg_quant_tables(int quality, uint16_t* luma, uint16_t* chroma) {
  if (quality < 1 || quality > 100 || !luma || !chroma) return ST_ERR_INVALID;
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    const long l = ((long)kBaseLuma[i] * scale + 50) / 100, c = ((long)kBaseChroma[i] * scale + 50) / 100;
    luma[i] = (uint16_t)(l < 1 ? 1 : (l > 255 ? 255 : l));
    chroma[i] = (uint16_t)(c < 1 ? 1 : (c > 255 ? 255 : c));
  }
  return ST_OK;
}

ST_JPEG_EXPORT int st_jpeg_encode_header_rst(int h, int w, int quality, int h_samp, int v_samp, int restart, uint8_t* buf, size_t cap, size_t* size) {
  char msg[160];
  int st = st_jpeg_enc_check_restart(restart, msg, sizeof msg);
  if (st == ST_OK) st = st_jpeg_enc_check(h, w, quality, h_samp, v_samp, msg, sizeof msg);
  if (st != ST_OK) return st;
  const size_t bytes = st_jpeg_enc_header_bytes(restart);
  if (size) *size = bytes;
  if (!buf || cap < bytes) return ST_ERR_INVALID;
  StJpegEncGeom g;
  st_jpeg_enc_geom(h, w, h_samp, v_samp, &g);
  uint16_t q[2][64];
  (void)st_jpeg_quant_tables(quality, q[0], q[1]);
  uint8_t* p = buf;
  auto put = [&p](int v) { *p++ = (uint8_t)v; };
  auto put2 = [&p](int v) { *p++ = (uint8_t)(v >> 8); *p++ = (uint8_t)v; };
  put2(0xFFD8);
  put2(0xFFE0); put2(16);   // JFIF 1.01, no units, 1:1 pixels, no thumbnail
  for (int c : {0x4A, 0x46, 0x49, 0x46, 0, 1, 1, 0}) put(c);   // "JFIF\0", version 1.01, density unit 0
  put2(1); put2(1); put(0); put(0);
  for (int t = 0; t < 2; ++t) {
    put2(0xFFDB); put2(67); put(t);
    for (int k = 0; k < 64; ++k) put(q[t][st_jpeg_enc_zigzag[k]]);
  }
  put2(0xFFC0); put2(17); put(8); put2(h); put2(w); put(3);
  put(1); put(h_samp << 4 | v_samp); put(0);
  put(2); put(0x11); put(1);
  put(3); put(0x11); put(1);
  for (const HuffSpec& s : kHuff) {
    put2(0xFFC4); put2(2 + 1 + 16 + s.nvals); put(s.cls_id);
    for (int i = 0; i < 16; ++i) put(s.bits[i]);
    for (int i = 0; i < s.nvals; ++i) put(s.vals[i]);
  }
  if (restart == ST_JPEG_RESTART_ROW) {
    put2(0xFFDD); put2(4); put2(g.mcols);   // one restart interval per MCU row
  }
  put2(0xFFDA); put2(12); put(3);
  put(1); put(0x00); put(2); put(0x11); put(3); put(0x11);
  put(0); put(63); put(0);
  return ST_OK;   // p - buf == st_jpeg_enc_header_bytes(restart): every segment above has a fixed length
}

ST_JPEG_EXPORT int st_jpeg_encode_header(int h, int w, int quality, int h_samp, int v_samp, uint8_t* buf, size_t cap, size_t* size) {
  return st_jpeg_encode_header_rst(h, w, quality, h_samp, v_samp, ST_JPEG_RESTART_ROW, buf, cap, size);
}

ST_JPEG_EXPORT long long st_jpeg_encode_bound(int h, int w, int h_samp, int v_samp) {
  char msg[160];
  if (st_jpeg_enc_check(h, w, 50, h_samp, v_samp, msg, sizeof msg) != ST_OK) return -1;
  StJpegEncGeom g;
  st_jpeg_enc_geom(h, w, h_samp, v_samp, &g);
  // header, every interval at its worst case, an RST marker between intervals, EOI
  return (long long)kJpegEncHeaderBytes + (long long)g.mrows * (long long)g.mcols * g.bpm * (long long)kJpegEncBlockStuffed +
         2LL * (g.mrows - 1) + 2;
}

// ---- optimised Huffman tables: the host twins of k_jpeg_sym_stats and k_jpeg_opt_tables ------------------
int st_jpeg_enc_check_optimize(int optimize, char* msg, size_t msg_len) {
  msg[0] = 0;
  if (optimize != 0 && optimize != 1) {
    snprintf(msg, msg_len, "optimize %d is not supported (0 or 1)", optimize);
    return ST_ERR_INVALID;
  }
  return ST_OK;
}

ST_JPEG_EXPORT int st_jpeg_optimal_table(const uint64_t freq[256], uint8_t bits[16], uint8_t vals[256], int* nvals) {
  if (!freq || !bits || !vals || !nvals) return ST_ERR_INVALID;
  StJpegOptWork w;
  // a code of more than 32 bits before the limiting: libjpeg stops there; the table returned is valid but not optimal
  return st_jpeg_opt_table_serial(freq, &w, bits, vals, nvals) ? ST_ERR_UNSUPPORTED : ST_OK;
}

ST_JPEG_EXPORT int st_jpeg_optimal_dht(const uint64_t freq[256], int table, uint8_t* buf, size_t cap, size_t* size, uint32_t* codes) {
  if (!freq || table < 0 || table >= kJpegOptTables) return ST_ERR_INVALID;
  StJpegOptWork w;
  uint8_t bits[16], vals[256];
  int nvals = 0;
  (void)st_jpeg_opt_table_serial(freq, &w, bits, vals, &nvals);
  const size_t bytes = (size_t)st_jpeg_opt_dht_bytes(nvals);
  if (size) *size = bytes;
  if (!buf || cap < bytes) return ST_ERR_INVALID;
  for (size_t i = 0; i < bytes; ++i) buf[i] = st_jpeg_opt_dht_byte(bits, vals, nvals, st_jpeg_opt_class_id(table), (int)i);
  if (codes) st_jpeg_opt_codes(bits, vals, nvals, codes, st_jpeg_opt_tab_words(table));
  return ST_OK;
}

ST_JPEG_EXPORT int st_jpeg_symbol_stats(const int16_t* coef, size_t cap, int h, int w, int h_samp, int v_samp, int restart, uint64_t* freq) {
  char msg[160];
  int st = st_jpeg_enc_check_restart(restart, msg, sizeof msg);
  if (st == ST_OK) st = st_jpeg_enc_check(h, w, 50, h_samp, v_samp, msg, sizeof msg);
  if (st != ST_OK) return st;
  if (!coef || !freq) return ST_ERR_INVALID;
  StJpegEncGeom g;
  st_jpeg_enc_geom(h, w, h_samp, v_samp, &g);
  const size_t luma_blocks = (size_t)g.mrows * v_samp * g.mcols * h_samp, chroma_blocks = (size_t)g.mrows * g.mcols;
  if (cap < (luma_blocks + 2 * chroma_blocks) * 64) return ST_ERR_INVALID;
  memset(freq, 0, sizeof(uint64_t) * kJpegOptTables * 256);
  int pred[3] = {0, 0, 0};
  auto block = [&](const int16_t* b, int comp) {
    uint64_t* f = freq + (comp == 0 ? 0 : 2) * 256;   // DC table of the component; its AC table follows
    const int diff = (int)b[0] - pred[comp];
    pred[comp] = b[0];
    st_jpeg_opt_block_symbols([b](int k) { return (int)b[st_jpeg_enc_zigzag[k]]; }, diff, [f](int ac, int sym) { f[ac * 256 + sym]++; });
  };
  for (int my = 0; my < g.mrows; ++my) {
    if (restart == ST_JPEG_RESTART_ROW) pred[0] = pred[1] = pred[2] = 0;
    for (int mx = 0; mx < g.mcols; ++mx) {
      for (int k = 0; k < h_samp * v_samp; ++k) {
        const size_t by = (size_t)my * v_samp + k / h_samp, bx = (size_t)mx * h_samp + k % h_samp;
        block(coef + (by * ((size_t)g.mcols * h_samp) + bx) * 64, 0);
      }
      for (int c = 0; c < 2; ++c) block(coef + (luma_blocks + c * chroma_blocks + (size_t)my * g.mcols + mx) * 64, 1 + c);
    }
  }
  return ST_OK;
}

ST_JPEG_EXPORT long long st_jpeg_encode_bound_opt(int h, int w, int h_samp, int v_samp) {
  char msg[160];
  if (st_jpeg_enc_check(h, w, 50, h_samp, v_samp, msg, sizeof msg) != ST_OK) return -1;
  StJpegEncGeom g;
  st_jpeg_enc_geom(h, w, h_samp, v_samp, &g);
  // the header (four DHT segments of at most 12 / 162 symbols: never more than the 629 bytes), every block at 1665 bits stuffed
  return (long long)kJpegEncHeaderBytes + (long long)g.mrows * (long long)g.mcols * g.bpm * (long long)kJpegEncBlockStuffedOpt +
         2LL * (g.mrows - 1) + 2;
}
