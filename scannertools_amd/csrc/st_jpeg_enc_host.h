// Host side of the ImageEncoder op: argument checks, geometry, quantisation and Huffman tables, and the stream's header.
// Plain C++ (no HIP): st_jpeg_enc_host.cpp also compiles on its own under a host sanitizer.  Re-entrant, no state.
#ifndef ST_JPEG_ENC_HOST_H_
#define ST_JPEG_ENC_HOST_H_

#include <stddef.h>
#include <stdint.h>

// Geometry of a (h, w, 3) frame at luma sampling hs x vs (chroma 1 x 1).  An MCU holds hs * vs luma blocks (row-major), then
// one Cb and one Cr block; a restart interval is one MCU row.
struct StJpegEncGeom {
  int h, w, hs, vs;
  int mcols, mrows;   // MCUs per row, MCU rows (= restart intervals)
  int bpm;            // blocks per MCU: hs * vs + 2
  int nbx, nby;       // real luma blocks per row / column: ceil(w / 8), ceil(h / 8); blocks beyond them are padding blocks
  int cw, ch;         // the chroma components' extent in samples: ceil(w / hs), ceil(h / vs)
};

// Worst case of one coded block.  Bits: a DC code of at most 11 bits and 11 magnitude bits, then 63 AC codes of at most 16
// bits with 10 magnitude bits each (ZRL and EOB only ever replace coefficients by fewer bits): 22 + 63 * 26 = 1660 bits, under
// 208 bytes.  Every byte may be 0xFF and then takes a stuffed zero: 416 bytes.  The transform kernel clamps DC differences to
// 11 and AC values to 10 magnitude bits (values no 8-bit picture reaches), so the bound holds whatever the input.
constexpr int kJpegEncBlockBits = 1660;
constexpr size_t kJpegEncBlockBytes = 208;          // before stuffing
constexpr size_t kJpegEncBlockStuffed = 416;        // after

// ST_OK, or the status of the refusal with its cause in msg (msg_len > 0).
int st_jpeg_enc_check(int h, int w, int quality, int h_samp, int v_samp, char* msg, size_t msg_len);
// The same for the restart mode (ST_JPEG_RESTART_*): ST_ERR_INVALID names any other value.
int st_jpeg_enc_check_restart(int restart, char* msg, size_t msg_len);
// The same for `optimize` (0: the Annex K tables, 1: per-frame optimal tables): ST_ERR_INVALID names any other value.
int st_jpeg_enc_check_optimize(int optimize, char* msg, size_t msg_len);
void st_jpeg_enc_geom(int h, int w, int h_samp, int v_samp, StJpegEncGeom* g);
// Bytes of an interval's slot: its blocks at their stuffed worst case (the padding of the last byte only fills a byte counted
// already), a multiple of 16.
inline size_t st_jpeg_enc_slot_bytes(const StJpegEncGeom& g) { return ((size_t)g.mcols * g.bpm * kJpegEncBlockStuffed + 15) / 16 * 16; }
// Bytes of an MCU row's slot in a stream without restart markers: its blocks' bits unstuffed and unpadded, the last byte
// zero-filled (1660 bits are 207.5 bytes, so 208 per block cover the partial byte too), a multiple of 16.
inline size_t st_jpeg_enc_raw_slot_bytes(const StJpegEncGeom& g) { return ((size_t)g.mcols * g.bpm * kJpegEncBlockBytes + 15) / 16 * 16; }
// The Annex K Huffman tables as (code length << 16) | code, indexed by symbol: [0, 16) DC luma, [16, 32) DC chroma,
// [32, 288) AC luma, [288, 544) AC chroma; 0 for a symbol without a code.
constexpr int kJpegEncHuffWords = 544;
void st_jpeg_enc_huff(uint32_t* tab);
// position k of the zigzag scan -> index in the row-major block (T.81 figure A.6); a list, because the kernels need the table as
// a device constant of their own
#define ST_JPEG_ENC_ZIGZAG \
  0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63
extern const uint8_t st_jpeg_enc_zigzag[64];
constexpr size_t kJpegEncHeaderBytes = 629;    // SOI .. SOS of a stream with one restart interval per MCU row
constexpr size_t kJpegEncHeaderBytesNoRst = kJpegEncHeaderBytes - 6;   // ... of one without restart markers: no DRI segment
// restart: ST_JPEG_RESTART_ROW (0) or ST_JPEG_RESTART_NONE (1), checked by the caller
inline size_t st_jpeg_enc_header_bytes(int restart) { return restart == 0 ? kJpegEncHeaderBytes : kJpegEncHeaderBytesNoRst; }

#endif  // ST_JPEG_ENC_HOST_H_
