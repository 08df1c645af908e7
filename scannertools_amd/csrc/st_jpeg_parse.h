// Host side of the ImageDecoder op: marker parser and Huffman (entropy) decoder of baseline JPEG streams.
// Plain C++ (no HIP): st_jpeg_parse.cpp also compiles on its own under a host sanitizer.  Re-entrant: everything a call
// needs lives in its StJpegHeader; nothing is kept between calls.
#ifndef ST_JPEG_PARSE_H_
#define ST_JPEG_PARSE_H_

#include <stddef.h>
#include <stdint.h>

// One Huffman table: a 9-bit lookahead for the short codes, the canonical max-code walk for the longer ones.
struct StJpegHuff {
  uint16_t look[512];   // (code length << 8) | symbol of the code that prefixes these 9 bits; 0: longer than 9 bits
  int32_t maxcode[18];  // largest code of each length (-1: none); [17] ends the walk
  int32_t valoff[17];   // index into vals of the first code of each length, minus that code
  uint8_t vals[256];
};

enum { ST_JPEG_444 = 0, ST_JPEG_H2V1 = 1, ST_JPEG_H2V2 = 2, ST_JPEG_GRAY = 3 };

struct StJpegHeader {
  int h, w, ncomp;
  int hs[3], vs[3];            // sampling factors as the scan uses them (1 x 1 for a one-component stream)
  int tq[3], td[3], ta[3];     // table selectors per component
  int restart_interval;
  int mode;                    // ST_JPEG_*
  int mcux, mcuy;              // MCUs per row / column
  int bw[3], bh[3];            // blocks per row / column of each component's block-padded plane
  size_t scan_pos;             // first entropy-coded byte
  bool have_q[4], have_dc[4], have_ac[4];
  uint16_t quant[4][64];       // natural (row-major) order
  StJpegHuff dc[4], ac[4];
};

// Number of 8 x 8 blocks of component c / of the whole frame (component planes in SOF order, each in raster order).
inline size_t st_jpeg_comp_blocks(const StJpegHeader& hd, int c) { return (size_t)hd.bw[c] * hd.bh[c]; }
inline size_t st_jpeg_blocks(const StJpegHeader& hd) {
  size_t n = 0;
  for (int c = 0; c < hd.ncomp; ++c) n += st_jpeg_comp_blocks(hd, c);
  return n;
}

// Markers up to and including SOS.  Returns an st_status; `msg` (msg_len > 0) names the cause of anything but ST_OK.
int st_jpeg_parse_header(const uint8_t* buf, size_t size, StJpegHeader* hd, char* msg, size_t msg_len);
// The scan of a parsed stream into st_jpeg_blocks(hd) * 64 coefficients (the layout of st_jpeg_coefficients).
int st_jpeg_decode_scan(const uint8_t* buf, size_t size, const StJpegHeader& hd, int16_t* coef, char* msg, size_t msg_len);

// Restart intervals of a parsed stream: ceil(MCUs / restart_interval), 0 for a stream without DRI.
inline size_t st_jpeg_interval_count(const StJpegHeader& hd) {
  if (hd.restart_interval <= 0) return 0;
  const size_t mcus = (size_t)hd.mcux * hd.mcuy;
  return (mcus + (size_t)hd.restart_interval - 1) / (size_t)hd.restart_interval;
}
// One walk over the entropy-coded segment from hd.scan_pos for 0xFF bytes: `table` receives st_jpeg_interval_count(hd)
// (begin, end) pairs of offsets into buf, `end` on the 0xFF of the marker that ends the interval (or size).  Stops after the
// last interval the frame needs.  ST_ERR_UNSUPPORTED: no DRI, or size >= 4 GiB; ST_ERR_INVALID: too few intervals, or an
// RSTn out of sequence.
int st_jpeg_scan_intervals(const uint8_t* buf, size_t size, const StJpegHeader& hd, uint32_t* table, char* msg, size_t msg_len);

// Segments of a parsed stream (byte ranges decoded from a known state): its restart intervals, or ONE for a stream without DRI.
inline size_t st_jpeg_segment_count(const StJpegHeader& hd) { return hd.restart_interval > 0 ? st_jpeg_interval_count(hd) : 1; }
// `table` receives st_jpeg_segment_count(hd) (begin, end) pairs: st_jpeg_scan_intervals' with DRI; without, the scan from
// hd.scan_pos to the first marker that is neither FF00 nor a fill byte (or size).  ST_ERR_UNSUPPORTED: size >= 4 GiB.
int st_jpeg_segments(const uint8_t* buf, size_t size, const StJpegHeader& hd, uint32_t* table, char* msg, size_t msg_len);

// Decoding at 1/d (d = 2, 4, 8; m = 8 / d is libjpeg's min_DCT_scaled_size): jdmaster's inverse DCT size S of every component
// (doubled from m while the component's remaining upsampling factor stays whole in both directions) and the extent
// (dw, dh) of its reduced plane in samples.  d = 1 gives S = 8 and the component's own extent.
inline void st_jpeg_reduced_geom(const StJpegHeader& hd, int d, int S[3], int dw[3], int dh[3]) {
  const int m = 8 / d, hmax = hd.hs[0], vmax = hd.vs[0];   // luma carries the largest factors in every sampling accepted
  for (int c = 0; c < 3; ++c) {
    S[c] = dw[c] = dh[c] = 0;
    if (c >= hd.ncomp) continue;
    int s = m;
    while (s < 8 && (hmax * m) % (hd.hs[c] * s * 2) == 0 && (vmax * m) % (hd.vs[c] * s * 2) == 0) s *= 2;
    S[c] = s;
    dw[c] = (int)(((long long)hd.w * hd.hs[c] * s + (long long)hmax * 8 - 1) / ((long long)hmax * 8));
    dh[c] = (int)(((long long)hd.h * hd.vs[c] * s + (long long)vmax * 8 - 1) / ((long long)vmax * 8));
  }
}

#endif  // ST_JPEG_PARSE_H_
