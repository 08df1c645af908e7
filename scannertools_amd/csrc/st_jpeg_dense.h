// What the dense JPEG decoding kernels share: st_jpeg.hip (k_jpeg_idct, k_jpeg_color: full size) and st_jpeg_reduced.hip
// (the same two stages at scale 1/2, 1/4 and 1/8).  The frame header both read, their launch arguments, and the launcher
// of the reduced pair.
#ifndef ST_JPEG_DENSE_H_
#define ST_JPEG_DENSE_H_

#include <stddef.h>
#include <stdint.h>

struct st_ctx;

struct alignas(16) JpegFrameHdr {
  uint8_t* out;          // the frame's dense (h, w, channels) output
  int blk_off;           // the frame's first block within the sub-batch
  int nblk_y, nblk_c;    // blocks of the luma plane / of each chroma plane (0 for a one-component stream)
  int bw_y, bw_c;        // blocks per row of them
  int mode;              // ST_JPEG_*
  int dw, dh;            // the chroma planes' real extent in samples (at a reduced scale: of the reduced planes)
  int fancy;             // 1: triangle filter; 0: replication (dw <= 2; at a reduced scale also 1/8)
  // a reduced scale only (0 at full size, where the kernels do not read them)
  int s_y, s_c;          // inverse DCT size of the luma blocks / of the chroma blocks: 1, 2, 4 or 8 samples a side
  int ups;               // horizontal upsampling left for chroma: 1 or 2 (vertical: never at a reduced scale)
  int pad0[2];
  uint16_t quant[3][64];
  uint8_t pad1[64];
};
static_assert(sizeof(JpegFrameHdr) == 512, "one header is 512 bytes");

struct JpegArgsK {
  const uint8_t* slot;   // headers, then coefficients
  uint8_t* planes;
  int nf, h, w, channels;   // h, w: the frames written (at a reduced scale: the reduced size)
};

// Blocks of a frame that the one-lane-per-block 1 x 1 kernel transforms, and the span of blocks the LDS kernel covers (it
// starts behind the luma plane when that is 1 x 1).
inline void st_jpeg_reduced_counts(const JpegFrameHdr& fh, size_t* n1, size_t* nlds) {
  const size_t ny = (size_t)fh.nblk_y, nc = 2 * (size_t)fh.nblk_c;
  *n1 = fh.s_y == 1 ? (fh.s_c == 1 ? ny + nc : ny) : 0;
  *nlds = fh.s_y == 1 ? (fh.s_c > 1 ? nc : 0) : ny + nc;
}

// The reduced inverse DCTs and the upsampling + colour kernel of nfl frames (a.slot at the first one's header; a.h, a.w the
// reduced size), on the context's stream.  most1 / mostlds: the largest st_jpeg_reduced_counts over the frames; px: 16, 4 or 1
// output pixels per lane.
void st_jpeg_reduced_launch(st_ctx* ctx, const JpegArgsK& a, int nfl, size_t most1, size_t mostlds, int px);

#ifdef __HIPCC__
typedef short short8 __attribute__((ext_vector_type(8)));
typedef unsigned short ushort8 __attribute__((ext_vector_type(8)));

// One pass of jidctint's 8-point inverse DCT (CONST_BITS 13): out = DESCALE(..., n), arithmetic shifts.
__device__ __forceinline__ void idct_pass(const int* i, int* o, int n) {
  int z1 = (i[2] + i[6]) * 4433;
  const int t2 = z1 - i[6] * 15137, t3 = z1 + i[2] * 6270;
  const int t0 = (i[0] + i[4]) * 8192, t1 = (i[0] - i[4]) * 8192;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int a = i[7], b = i[5], c = i[3], d = i[1];
  z1 = a + d;
  int z2 = b + c, z3 = a + c, z4 = b + d;
  const int z5 = (z3 + z4) * 9633;
  a *= 2446; b *= 16819; c *= 25172; d *= 12299;
  z1 *= -7373; z2 *= -20995;
  z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
  a += z1 + z3; b += z2 + z4; c += z2 + z3; d += z1 + z4;
  const int r = 1 << (n - 1);
  o[0] = (t10 + d + r) >> n; o[7] = (t10 - d + r) >> n;
  o[1] = (t11 + c + r) >> n; o[6] = (t11 - c + r) >> n;
  o[2] = (t12 + b + r) >> n; o[5] = (t12 - b + r) >> n;
  o[3] = (t13 + a + r) >> n; o[4] = (t13 - a + r) >> n;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// jdcolor's YCbCr -> RGB in 16 fractional bits
__device__ __forceinline__ void ycc_rgb(int Y, int Cb, int Cr, int* rgb) {
  const int cb = Cb - 128, cr = Cr - 128;
  rgb[0] = clamp255(Y + ((91881 * cr + 32768) >> 16));
  rgb[1] = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  rgb[2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
}
#endif  // __HIPCC__

#endif  // ST_JPEG_DENSE_H_
