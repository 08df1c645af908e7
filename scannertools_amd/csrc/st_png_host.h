// PNG on the host: the container parser, the zlib-stream inflater and the CPU twin of the kernels of st_png.hip.
// Host-only C++ (st_png_host.cpp); everything here is re-entrant.
#ifndef ST_PNG_HOST_H_
#define ST_PNG_HOST_H_

#include <cstddef>
#include <cstdint>
#include <vector>

#include "scannertools_hip.h"

// how a frame leaves the reconstructed scanlines
enum {
  ST_PNG_DIRECT = 0,     // gray 8, RGB 8 without tRNS, RGBA 8: the scanlines are the frame
  ST_PNG_GRAY_BITS = 1,  // gray at depth 1 / 2 / 4 -> 1 channel, scaled
  ST_PNG_PALETTE = 2,    // palette at depth 1 / 2 / 4 / 8 -> 3 or 4 channels
  ST_PNG_GRAY_ALPHA = 3, // (g, a) -> (g, g, g, a)
  ST_PNG_RGB_KEY = 4     // RGB + tRNS -> R, G, B, A
};

struct StPngIdat { size_t off, len; };   // one IDAT chunk's data within the stream

struct StPngHeader {
  int h, w, channels;      // of the decoded frame
  int color_type, bit_depth, interlace;
  int npal, ntrns;         // entries of PLTE / bytes of tRNS; 0: no such chunk
  int has_trns;
  int bpp;                 // the filters' distance to the "left" byte: 1, 2, 3 or 4
  int rowbytes;            // bytes of a scanline without its filter byte
  int kind;                // ST_PNG_*
  uint8_t pal[256 * 4];    // R, G, B, A of every index; past the palette opaque black
  uint8_t key[3];          // the colour key of ST_PNG_RGB_KEY
  std::vector<StPngIdat> idat;   // full parse only
  size_t idat_bytes;
};

// Parses the signature and the chunks: up to the first IDAT (full = false, st_png_probe) or to IEND (full = true: the chunk
// order, the IDAT list, the CRCs of IHDR, PLTE, tRNS and IEND).  The IDAT chunks' CRCs run over nearly all of a stream's bytes:
// st_png_inflate_rows checks them, on the thread that inflates the stream.  ST_OK, ST_ERR_UNSUPPORTED or ST_ERR_INVALID with
// the cause in msg.
int st_png_parse(const uint8_t* buf, size_t size, bool full, StPngHeader* hd, char* msg, size_t msg_len);
void st_png_fill_info(const StPngHeader& hd, st_png_info* info);
inline size_t st_png_raw_bytes(const StPngHeader& hd) { return (size_t)hd.h * (1 + (size_t)hd.rowbytes); }
inline size_t st_png_frame_bytes(const StPngHeader& hd) { return (size_t)hd.h * hd.w * hd.channels; }

// Inflates the zlib stream that the pieces (off, len) of base form when joined, into dst[0, cap).  No allocation; never writes
// past cap.  ST_OK or ST_ERR_INVALID with the cause in msg (may be null).
int st_zlib_inflate_pieces(const uint8_t* base, const StPngIdat* pieces, size_t npieces, uint8_t* dst, size_t cap, size_t* produced,
                           char* msg, size_t msg_len);
// Stage 1 of a parsed stream: checks the IDAT chunks' CRCs, inflates into raw[0, st_png_raw_bytes) exactly and checks every
// row's filter type.
int st_png_inflate_rows(const uint8_t* buf, const StPngHeader& hd, uint8_t* raw, char* msg, size_t msg_len);

// The CPU twin of k_png_unfilter: raw -> recon (h x rowbytes, dense).  Then of k_png_expand: recon -> frame.
void st_png_unfilter_host(const StPngHeader& hd, const uint8_t* raw, uint8_t* recon);
void st_png_expand_host(const StPngHeader& hd, const uint8_t* recon, uint8_t* frame);

#endif  // ST_PNG_HOST_H_
