// Frame statistics of interleaved U8x3 frames: the arithmetic of the legacy op library's BrightnessCPP, ContrastCPP and
// SharpnessCPP kernels (/root/reference/scannertools/scannertools/old/cpp_ops/imgproc.cpp:50-175) and of their Python twins
// Brightness, Contrast and Sharpness (old/imgproc.py:11-37).
//
// Contract.  A frame is U8 (h, w, 3) RGB with no row padding; N = h*w.
//   Y    = (R*4899 + G*9617 + B*1868 + 8192) >> 14, the luma byte of cv::cvtColor(COLOR_RGB2YUV) (the constants and rounding
//          of ConvertColor's COLOR_RGB2YUV, st_imgproc.hip).
//   L_c  = cv::Laplacian(frame, CV_64F) at its defaults (ksize 1, scale 1, delta 0, BORDER_DEFAULT), per channel c:
//          I(y-1,x) + I(y+1,x) + I(y,x-1) + I(y,x+1) - 4 I(y,x) with reflect-101 indices (-1 -> 1, h -> h-2); on an axis of
//          length 1 the neighbour is the pixel itself.  An integer in [-1020, 1020].
//   Moments per frame, eight exact integers, in this order (ST_FM_*): SY = sum Y, QY = sum Y^2, S_R, S_G, S_B = sum L_c,
//   Q_R, Q_G, Q_B = sum L_c^2.
// The six outputs are fixed double expressions of the moments (no FMA contraction; the library builds with -ffp-contract=off):
//   BrightnessCPP  (float)(SY * (1.0/N))                         cv::mean(yuv)[0], OpenCV scales by 1./nz
//   Brightness     SY / N                                        np.mean(frame, (0,1))[0]
//   ContrastCPP    (float)sqrt(var_Y)                            var_Y = (N*QY - SY^2) / (N*N), the numerator an exact integer
//   Contrast       sqrt(var_Y)                                   np.sqrt(np.mean((I - mean)**2))
//   SharpnessCPP   m = S_c*(1.0/N), sd = sqrt(max(Q_c*(1.0/N) - m*m, 0)), v_c = sd*sd; (float)((v_R + v_G + v_B) / 3.0)
//                                                                meanStdDev + pow(., 2) + /3.f (imgproc.cpp:157-165)
//   Sharpness      (3N * sum Q_c - (sum S_c)^2) / ((3N)*(3N))    cv2.Laplacian(frame, CV_64F).var()
// Deviation (documented, not reproduced): ContrastCPP accumulates ((float)Y - (float)mean)^2 in ONE float32 running sum over
// N terms (imgproc.cpp:113-121), which depends on the order and drifts; this returns the exactly rounded population standard
// deviation, which is also what the Python Contrast op gives (bound: DESIGN.md, tests/test_frame_stats.py).
//
// Kernel.  One launch covers the whole call (frames on grid.y, at most 65 535 per launch).  A workgroup owns a band of rows of
// one frame.  It streams the band's bytes, plus one halo row above and one below when the Laplacian is asked for, with 16-byte
// loads into a ring buffer in LDS that holds a rolling window of a little more than three rows, so each byte comes from HBM
// once (halo rows aside).  A lane then takes 16 consecutive bytes of the band per step and reads its neighbours (+-3 bytes
// across the row, +-3w bytes to the rows above and below) from the ring.  A step is 16 * 384 bytes, a multiple of 3, so a
// lane's byte positions keep their channel for the whole band: its sums go into three position-group accumulators that are
// assigned to channels once, at the end.  Per-lane partials are 32-bit (the band height is capped so that they cannot
// overflow), the workgroup reduces them to 64 bits and adds its eight values into the frame's int64 record with 64-bit
// atomics; the call zeroes the record on the stream first.  Integer sums do not depend on the order: the result is the same
// bit for bit whatever the batch, the launch split or the workgroup order.
#include <hip/hip_ext.h>

#include "st_internal.h"

namespace {

constexpr int FM_T = 384;                 // threads per workgroup (6 waves)
constexpr int FM_STEP = 16 * FM_T;        // bytes per step: 6144, a multiple of 3
constexpr int FM_MAX_STEPS = 512;         // steps per band: keeps every 32-bit per-lane partial exact (see fm_band_rows)
constexpr int FM_MAX_RING_LOG2 = 17;      // 128 KB of LDS: rows of up to 59 360 bytes (w <= 19 786) with the Laplacian

typedef unsigned u4nt __attribute__((ext_vector_type(4)));

struct FrameSrc {
  const uint8_t* const* ptrs;  // device table of frame pointers, or null
  const uint8_t* base;         // strided stream
  size_t stride;
};

// luma byte of one pixel (COLOR_RGB2YUV, 14-bit fixed point)
__device__ __forceinline__ unsigned luma(unsigned r, unsigned g, unsigned b) { return (r * 4899u + g * 9617u + b * 1868u + 8192u) >> 14; }

__device__ __forceinline__ unsigned byte_of(const unsigned* d, int j) { return (d[j >> 2] >> (8 * (j & 3))) & 0xffu; }

template <int WHAT, int RING_LOG2>
__global__ __launch_bounds__(FM_T) void k_frame_moments(FrameSrc src, int h, int w, int band_rows, unsigned long long* __restrict__ out) {
  constexpr int RING = 1 << RING_LOG2;
  constexpr unsigned DMASK = (RING >> 2) - 1;   // ring index mask in dwords
  constexpr bool LUMA = WHAT & ST_FM_LUMA, LAP = WHAT & ST_FM_LAPLACIAN;
  __shared__ uint4 ring4[RING / 16];
  __shared__ unsigned long long red[FM_T / 64][8];
  unsigned* ring = reinterpret_cast<unsigned*>(ring4);
  const int tid = threadIdx.x;
  const int frame = blockIdx.y;
  const uint8_t* p = src.ptrs ? src.ptrs[frame] : src.base + (size_t)frame * src.stride;
  p = st_gl(p);
  const int fs = (int)((uintptr_t)p & 15);      // frame start inside its first 16-byte block
  const uint8_t* a0 = p - fs;                   // aligned origin: "aligned" positions below are bytes from a0
  const long long R = 3LL * w, N3 = R * h;
  const int y0 = blockIdx.x * band_rows;
  const int y1 = min(y0 + band_rows, h);
  // frame byte ranges: computed [cs, ce), loaded [ls, le) (halo rows for the Laplacian)
  const long long cs = y0 * R, ce = y1 * R;
  const long long ls = LAP ? (y0 > 0 ? (y0 - 1) * R : 0) : cs, le = LAP ? (y1 < h ? (y1 + 1) * R : N3) : ce;
  const long long lv0 = (ls + fs) >> 4, lv1 = (le + fs + 15) >> 4;    // vectors loaded
  const long long cv0 = (cs + fs) >> 4, cv1 = (ce + fs + 15) >> 4;    // vectors computed
  // a vector's Laplacian reads up to R + 4 bytes past its end (rounded to whole dwords): this many vectors ahead
  const long long ahead = LAP ? (R + 4 + 15) / 16 + 1 : 1;
  const unsigned su = (unsigned)((-R) & 3), sd = (unsigned)(R & 3);   // byte shifts of the rows above / below within a dword

  // lane's first vector and the channel of its byte 0 (fixed for the whole band: the step is a multiple of 3)
  const long long a_first = (cv0 + tid) * 16;
  const int ph = (int)(((a_first - fs) % 3 + 3) % 3);

  // column (byte within the row) of the lane's byte 0, advanced by one step per iteration instead of divided out each time
  const int Ri = (int)R;
  int col0 = (int)(((a_first - fs) % R + R) % R);
  const int step_col = (int)(FM_STEP % R);

  unsigned s_g[3] = {0, 0, 0}, q_g[3] = {0, 0, 0};   // Laplacian sum / sum of squares per position group (position mod 3)
  unsigned sy = 0, qy = 0;

  long long loaded = lv0;
  for (long long c0 = cv0; c0 < cv1; c0 += FM_T) {
    long long need = c0 + FM_T + ahead;
    if (need > lv1) need = lv1;
    // fill the ring up to `need` (16-byte loads; the two vectors that hold bytes outside the frame byte by byte)
    for (; loaded < need; loaded += FM_T) {
      const long long v = loaded + tid;
      if (v < lv1) {
        uint4 q;
        const long long b0 = v * 16 - fs;   // frame index of the vector's first byte
        if (b0 >= 0 && b0 + 16 <= N3) {
          const u4nt t = __builtin_nontemporal_load(reinterpret_cast<const u4nt*>(a0) + v);   // every byte is read once
          q = make_uint4(t.x, t.y, t.z, t.w);
        } else {
          unsigned d[4] = {0, 0, 0, 0};
          for (int j = 0; j < 16; ++j)
            if (b0 + j >= 0 && b0 + j < N3) d[j >> 2] |= (unsigned)p[b0 + j] << (8 * (j & 3));
          q = make_uint4(d[0], d[1], d[2], d[3]);
        }
        ring4[(unsigned)v & (RING / 16 - 1)] = q;
      }
    }
    __syncthreads();
    const long long v = c0 + tid;
    if (v < cv1) {
      const long long a = v * 16;          // aligned position of byte 0
      const long long i0 = a - fs;         // its frame index
      const unsigned da = (unsigned)(a >> 2);
      unsigned c[6];                       // bytes a-4 .. a+19 of this row
#pragma unroll
      for (int k = 0; k < 6; ++k) c[k] = ring[(da - 1 + k) & DMASK];
      // interior: all 16 bytes in the band, none in the first or last row or column (and the pixel that starts at byte 15
      // lies in the band too, since band edges are pixel edges)
      const bool interior = i0 >= cs && i0 + 16 <= ce && i0 >= R && i0 + 16 <= N3 - R && col0 >= 3 && col0 + 19 <= R;
      if (LAP) {
        unsigned u[4], d[4];
        {
          const unsigned du = (unsigned)((a - R) >> 2), dd = (unsigned)((a + R) >> 2);
          unsigned ru[5], rd[5];
#pragma unroll
          for (int k = 0; k < 5; ++k) { ru[k] = ring[(du + k) & DMASK]; rd[k] = ring[(dd + k) & DMASK]; }
#pragma unroll
          for (int k = 0; k < 4; ++k) { u[k] = __builtin_amdgcn_alignbyte(ru[k + 1], ru[k], su); d[k] = __builtin_amdgcn_alignbyte(rd[k + 1], rd[k], sd); }
        }
        if (interior) {
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int cc = (int)byte_of(c + 1, j);
            const int l = (int)(byte_of(c, j + 1) + byte_of(c, j + 7) + byte_of(u, j) + byte_of(d, j)) - 4 * cc;
            s_g[j % 3] += (unsigned)l;
            q_g[j % 3] += (unsigned)(l * l);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const long long i = i0 + j;
            if (i < cs || i >= ce) continue;
            int col = col0 + j;
            if (col >= Ri) col %= Ri;
            const unsigned cc = byte_of(c + 1, j);
            unsigned lf = byte_of(c, j + 1), rt = byte_of(c, j + 7), up = byte_of(u, j), dn = byte_of(d, j);
            if (w == 1) { lf = cc; rt = cc; }
            else if (col < 3) lf = rt;
            else if (col >= Ri - 3) rt = lf;
            if (h == 1) { up = cc; dn = cc; }
            else if (i < R) up = dn;
            else if (i >= N3 - R) dn = up;
            const int l = (int)(lf + rt + up + dn) - 4 * (int)cc;
            s_g[j % 3] += (unsigned)l;
            q_g[j % 3] += (unsigned)(l * l);
          }
        }
      }
      if (LUMA) {
        // pixels that start in this lane's 16 bytes: at j0, j0 + 3, ... (j0 = 0 when byte 0 is a red byte)
        const unsigned j0 = (unsigned)((3 - ph) % 3);
        unsigned s[5];                         // bytes j0 .. j0 + 19
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] = __builtin_amdgcn_alignbyte(c[k < 4 ? k + 2 : 5], c[k + 1], j0);   // bytes 18, 19 unused
        if (interior) {
#pragma unroll
          for (int m = 0; m < 6; ++m) {
            const unsigned y = luma(byte_of(s, 3 * m), byte_of(s, 3 * m + 1), byte_of(s, 3 * m + 2));
            const unsigned take = (m < 5 || j0 == 0) ? 1u : 0u;   // a sixth pixel starts here only at byte 15
            sy += y * take;
            qy += y * y * take;
          }
        } else {
#pragma unroll
          for (int m = 0; m < 6; ++m) {
            const long long i = i0 + j0 + 3 * m;
            if (3 * m + j0 > 15 || i < cs || i >= ce) continue;
            const unsigned y = luma(byte_of(s, 3 * m), byte_of(s, 3 * m + 1), byte_of(s, 3 * m + 2));
            sy += y;
            qy += y * y;
          }
        }
      }
    }
    __syncthreads();   // the next fill overwrites ring slots this step read
    col0 += step_col;
    if (col0 >= Ri) col0 -= Ri;
  }

  // position groups -> channels: byte position j of this lane has channel (ph + j) % 3
  long long acc[8];
  acc[ST_FM_SY] = sy;
  acc[ST_FM_QY] = qy;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int g = (ch - ph + 3) % 3;
    const unsigned sg = g == 0 ? s_g[0] : g == 1 ? s_g[1] : s_g[2];
    const unsigned qg = g == 0 ? q_g[0] : g == 1 ? q_g[1] : q_g[2];
    acc[ST_FM_S_R + ch] = (long long)(int)sg;
    acc[ST_FM_Q_R + ch] = (long long)qg;
  }
  // workgroup reduction in 64 bits: wave shuffles, then one row per wave in LDS
#pragma unroll
  for (int k = 0; k < 8; ++k)
    for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_down(acc[k], off, 64);
  if ((tid & 63) == 0)
    for (int k = 0; k < 8; ++k) red[tid >> 6][k] = (unsigned long long)acc[k];
  __syncthreads();
  if (tid < 8) {
    unsigned long long t = 0;
    for (int wv = 0; wv < FM_T / 64; ++wv) t += red[wv][tid];
    const bool used = (tid < 2) ? LUMA : LAP;
    if (used && t) atomicAdd(out + (size_t)frame * 8 + tid, t);
  }
}

// (unsigned) 128-bit integer hi:lo to the nearest double (ties to even): the top 64 bits with a sticky bit, scaled
__device__ double u128_to_double(unsigned long long hi, unsigned long long lo) {
  if (hi == 0) return (double)lo;
  const int k = 64 - __clzll((long long)hi);                  // bits of hi, 1..64
  unsigned long long top = k == 64 ? hi : (hi << (64 - k)) | (lo >> k);
  const unsigned long long rest = k == 64 ? lo : lo << (64 - k);
  if (rest) top |= 1;                                          // sticky: below the rounding position of a 53-bit mantissa
  return ldexp((double)top, k);
}

// a*b - c*d for non-negative 64-bit a, b, c, d with a*b >= c*d, exactly, as a double rounded once
__device__ double exact_diff_of_products(unsigned long long a, unsigned long long b, unsigned long long c, unsigned long long d) {
  const unsigned long long plo = a * b, phi = __umul64hi(a, b);
  const unsigned long long qlo = c * d, qhi = __umul64hi(c, d);
  const unsigned long long lo = plo - qlo;
  const unsigned long long hi = phi - qhi - (plo < qlo ? 1 : 0);
  return u128_to_double(hi, lo);
}

// statistic `kind` (ST_FS_*) of one moments record r for frames of N pixels, as a double (the *_CPP kinds are then rounded to float)
__device__ double fs_value(const long long* r, long long N, int kind) {
  const double dN = (double)N;
  double v = 0.0;
  switch (kind) {
    case ST_FS_BRIGHTNESS_CPP: v = (double)r[ST_FM_SY] * __ddiv_rn(1.0, dN); break;
    case ST_FS_BRIGHTNESS: v = __ddiv_rn((double)r[ST_FM_SY], dN); break;
    case ST_FS_CONTRAST_CPP:
    case ST_FS_CONTRAST: {
      const double num = exact_diff_of_products((unsigned long long)N, (unsigned long long)r[ST_FM_QY], (unsigned long long)r[ST_FM_SY],
                                                (unsigned long long)r[ST_FM_SY]);
      v = __dsqrt_rn(__ddiv_rn(num, dN * dN));
      break;
    }
    case ST_FS_SHARPNESS_CPP: {
      const double scale = __ddiv_rn(1.0, dN);
      double t = 0.0;
      for (int ch = 0; ch < 3; ++ch) {
        const double mean = (double)r[ST_FM_S_R + ch] * scale;
        double var = (double)r[ST_FM_Q_R + ch] * scale - mean * mean;
        var = var > 0.0 ? var : 0.0;
        const double sdv = __dsqrt_rn(var);
        t = t + sdv * sdv;
      }
      v = __ddiv_rn(t, 3.0);
      break;
    }
    case ST_FS_SHARPNESS: {
      const long long s = r[ST_FM_S_R] + r[ST_FM_S_G] + r[ST_FM_S_B];
      const unsigned long long q = (unsigned long long)r[ST_FM_Q_R] + (unsigned long long)r[ST_FM_Q_G] + (unsigned long long)r[ST_FM_Q_B];
      const unsigned long long as = (unsigned long long)(s < 0 ? -s : s);
      const double num = exact_diff_of_products((unsigned long long)(3 * N), q, as, as);
      const double d3 = (double)(3 * N);
      v = __ddiv_rn(num, d3 * d3);
      break;
    }
  }
  return v;
}
__device__ __forceinline__ void fs_store(void* out, size_t i, int kind, double v) {
  if (kind <= ST_FS_SHARPNESS_CPP) reinterpret_cast<float*>(out)[i] = (float)v;
  else reinterpret_cast<double*>(out)[i] = v;
}

__global__ __launch_bounds__(256) void k_frame_stats_finish(const long long* __restrict__ m, int n, long long N, int kind, void* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  fs_store(out, (size_t)i, kind, fs_value(m + (size_t)i * 8, N, kind));
}

// ---- SharpnessBBox: boxes of a frame, resized to ST_BBOX_SIDE x ST_BBOX_SIDE, to Laplacian moments -----------------------------
// Contract (imgproc.cpp:177-234, old/imgproc.py:44-54): per box, the region frame[y1:y2, x1:x2] treated as an image of its own
// is resized to 200 x 200 at INTER_LINEAR with the Resize op's arithmetic (the device functions of st_internal.h: an equal size
// is a copy, an exact 2 x 2 decimation the rounded mean of four, else 11-bit fixed-point two-tap rows and columns whose taps
// clamp inside the region), and the moments S_c, Q_c of the reflect-101 Laplacian of that image are the record.
//
// Kernel.  One workgroup of 1024 threads per box.  The resized image is 120 000 bytes and is built in LDS (rows 640 bytes
// apart), never in HBM; after a barrier the same workgroup takes the Laplacian out of LDS, reduces per-lane 32-bit partials
// (at most 40 values of L^2 <= 1020^2 per lane and channel) to 64 bits and writes the box's record, and, if asked, the
// finished statistic: one writer per record, no atomics, no zeroing pass.  128 KB of LDS means one workgroup per CU, and a
// whole box keeps one CU busy for about 50 us (the pass is bound by that CU's vector ALU), so a call with fewer boxes than
// CUs cuts every box into up to 10 bands of rows, one workgroup each (its band plus a halo row on each side), which write
// their six sums to scratch; a second, tiny launch (k_bbox_finish) adds them up and finishes.  Measured on 1080p frames
// (DESIGN.md 4.11): one box 50.9 us as one workgroup, against 38.3 us for the composed older entry points; banded, see there.
//   copy (200 x 200 box): a row is fetched with 16-byte loads at the source's own alignment and lands in its LDS row at the
//     same offset modulo 16, so no byte is shifted on the way in; the Laplacian pass adds the row's offset instead.
//   2 x 2 mean (400 x 400): four output pixels per step, 24 contiguous bytes of two rows as unaligned dwords (the Resize kernel's).
//   linear (everything else): per-column and per-row taps and weights are computed once per box into LDS, then four output
//     pixels per step, each tap pair as two unaligned dwords (the Resize kernel's); a 1080p-wide box reads 6 bytes in 29.
// The host has checked every box against the frame (bb_plan) before the launch; the kernel trusts its table.
constexpr int BB_T = 1024;
constexpr int BB_S = ST_BBOX_SIDE;
constexpr int BB_ROW = 3 * BB_S;        // bytes of an image row
constexpr int BB_PITCH = 640;           // LDS row pitch: the row + up to 15 bytes of source misalignment, a multiple of 16
constexpr int BB_G = BB_S / 4;          // groups of four pixels per row
constexpr int BB_MAX_BANDS = 10;        // a box is cut into at most this many bands of rows (calls with few boxes)
constexpr int BB_VEC = (BB_ROW + 15 + 15) / 16;   // 16-byte vectors that can hold bytes of one misaligned row: 39
static_assert(BB_S % 4 == 0 && BB_PITCH % 16 == 0 && BB_VEC * 16 <= BB_PITCH, "SharpnessBBox LDS layout");

struct BoxK {
  int frame, x1, y1, bw, bh, mode;   // mode: RS_COPY, RS_AREA2 or RS_LINEAR (st_rs_linear_mode on the host)
  double scale_x, scale_y;           // cv::resize's source / destination ratios (st_rs_plan_scales on the host)
};

// bands == 1: the workgroup owns the whole image and writes the record (out) and / or the statistic (stat_out).  bands > 1
// (calls with fewer boxes than CUs): workgroup box * bands + j builds rows j * band_rows - 1 .. (j + 1) * band_rows of the image
// (its band and a halo row on each side) and writes its six sums to part[box * bands + j]; k_bbox_finish adds them up.
__global__ __launch_bounds__(BB_T) void k_bbox_moments(FrameSrc src, int h, int w, const BoxK* __restrict__ boxes, int bands, int band_rows,
                                                       unsigned long long* __restrict__ part, unsigned long long* __restrict__ out, int kind,
                                                       void* stat_out) {
  __shared__ uint4 img4[1 + BB_S * BB_PITCH / 16 + 1];   // 16 bytes of slack before and after: windows reach 3 bytes outside a row
  __shared__ int tx_ofs[BB_S], ty_y0[BB_S], ty_y1[BB_S];
  __shared__ unsigned tx_a[BB_S], ty_b[BB_S];            // a0 | a1 << 16, b0 | b1 << 16 (weights are 0 .. 2048)
  __shared__ unsigned char tx_flags[BB_S];               // 1: two taps, 2: 8 bytes from the first tap stay inside the region row
  __shared__ unsigned long long red[BB_T / 64][6];
  unsigned* img = reinterpret_cast<unsigned*>(img4 + 1);
  const int tid = threadIdx.x;
  const size_t box = blockIdx.x / (unsigned)bands;
  const int r0 = (int)(blockIdx.x % (unsigned)bands) * band_rows, r1 = min(r0 + band_rows, BB_S);   // rows this workgroup sums
  const int fa = max(r0 - 1, 0), fb = min(r1 + 1, BB_S);   // rows it builds: reflect-101 keeps the neighbours of rows 0 and 199 inside
  const BoxK b = boxes[box];
  const uint8_t* p = src.ptrs ? src.ptrs[b.frame] : src.base + (size_t)b.frame * src.stride;
  p = st_gl(p);
  const long long frow = 3LL * w, N3 = frow * h;
  const long long i0 = ((long long)b.y1 * w + b.x1) * 3;   // frame index of the region's first byte
  const uint8_t* reg = p + i0;
  // copy path: LDS row r starts (sa + r * ss) & 15 bytes into its pitch, the source row's own offset in its 16-byte block
  const unsigned fs = (unsigned)((uintptr_t)p & 15);
  const unsigned sa = b.mode == RS_COPY ? (unsigned)((i0 + fs) & 15) : 0u, ss = b.mode == RS_COPY ? (unsigned)(frow & 15) : 0u;

  if (b.mode == RS_COPY) {
    for (int idx = tid; idx < (fb - fa) * BB_VEC; idx += BB_T) {
      const int r = fa + idx / BB_VEC, k = idx % BB_VEC;
      const long long ir = i0 + r * frow;                       // frame index of the row's first byte
      const long long v0 = ((ir + fs) & ~15LL) - fs + 16 * k;   // frame index of this vector's first byte (may be negative)
      if (v0 >= ir + BB_ROW) continue;                          // past the row
      uint4 q;
      if (v0 >= 0 && v0 + 16 <= N3) {
        const u4nt t = *reinterpret_cast<const u4nt*>(p + v0);
        q = make_uint4(t.x, t.y, t.z, t.w);
      } else {   // the vector holds bytes outside the frame: those stay unread
        unsigned d[4] = {0, 0, 0, 0};
        for (int j = 0; j < 16; ++j)
          if (v0 + j >= 0 && v0 + j < N3) d[j >> 2] |= (unsigned)p[v0 + j] << (8 * (j & 3));
        q = make_uint4(d[0], d[1], d[2], d[3]);
      }
      img4[1 + r * (BB_PITCH / 16) + k] = q;
    }
  } else if (b.mode == RS_AREA2) {
    for (int idx = tid; idx < (fb - fa) * BB_G; idx += BB_T) {
      const int r = fa + idx / BB_G, g = idx % BB_G;
      const uint8_t* S0 = reg + (size_t)(2 * r) * frow + 24 * g;
      unsigned o[3];
      rs_area2_4px_c3(S0, S0 + frow, o);
      unsigned* d = img + r * (BB_PITCH / 4) + 3 * g;
      d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
    }
  } else {
    if (tid < BB_S) {
      int sx;
      const float fx = rs_linear_coord(tid, b.scale_x, &sx);
      const RsTapX t = rs_linear_tap_x(sx, fx, b.bw);
      tx_ofs[tid] = t.sx * 3;
      tx_a[tid] = (unsigned)t.a0 | (unsigned)t.a1 << 16;
      tx_flags[tid] = (unsigned char)((t.two ? 1 : 0) | ((long long)t.sx * 3 + 8 <= 3LL * b.bw ? 2 : 0));
    } else if (tid >= 256 && tid < 256 + BB_S) {
      const int dy = tid - 256;
      int sy;
      const float fy = rs_linear_coord(dy, b.scale_y, &sy);
      const RsTapY t = rs_linear_tap_y(sy, fy, b.bh);
      ty_y0[dy] = t.y0; ty_y1[dy] = t.y1;
      ty_b[dy] = (unsigned)t.b0 | (unsigned)t.b1 << 16;
    }
    __syncthreads();
    for (int idx = tid; idx < (fb - fa) * BB_G; idx += BB_T) {
      const int r = fa + idx / BB_G, g = idx % BB_G;
      const uint8_t* __restrict__ R0 = reg + (size_t)ty_y0[r] * frow;
      const uint8_t* __restrict__ R1 = reg + (size_t)ty_y1[r] * frow;
      const int b0 = (int)(ty_b[r] & 0xffffu), b1 = (int)(ty_b[r] >> 16);
      unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = 4 * g + q;
        const unsigned a = tx_a[c], fl = tx_flags[c];
        rs_linear_px_c3(R0, R1, tx_ofs[c], (int)(a & 0xffffu), (int)(a >> 16), fl & 1, fl & 2, b0, b1, q, o);
      }
      unsigned* d = img + r * (BB_PITCH / 4) + 3 * g;
      d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
    }
  }
  __syncthreads();

  // Laplacian of the image in LDS, 12 bytes (four pixels) per step: a group starts at a multiple of 3, so byte j has channel j % 3
  int s_c[3] = {0, 0, 0};
  unsigned q_c[3] = {0, 0, 0};
  for (int idx = tid; idx < (r1 - r0) * BB_G; idx += BB_T) {
    const int r = r0 + idx / BB_G, g = idx % BB_G;
    const int ru = r == 0 ? 1 : r - 1, rd = r == BB_S - 1 ? BB_S - 2 : r + 1;   // reflect-101
    const int oc = r * BB_PITCH + (int)((sa + r * ss) & 15u) + 12 * g - 3;     // bytes -3 .. 14 of the group, this row
    const int ou = ru * BB_PITCH + (int)((sa + ru * ss) & 15u) + 12 * g;
    const int od = rd * BB_PITCH + (int)((sa + rd * ss) & 15u) + 12 * g;
    unsigned c[5], u[3], d[3];
    {
      unsigned rc[6], rr[4];
      const unsigned* wc = img + (oc >> 2);
#pragma unroll
      for (int k = 0; k < 6; ++k) rc[k] = wc[k];
#pragma unroll
      for (int k = 0; k < 5; ++k) c[k] = __builtin_amdgcn_alignbyte(rc[k + 1], rc[k], (unsigned)(oc & 3));
      const unsigned* wu = img + (ou >> 2);
#pragma unroll
      for (int k = 0; k < 4; ++k) rr[k] = wu[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) u[k] = __builtin_amdgcn_alignbyte(rr[k + 1], rr[k], (unsigned)(ou & 3));
      const unsigned* wd = img + (od >> 2);
#pragma unroll
      for (int k = 0; k < 4; ++k) rr[k] = wd[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) d[k] = __builtin_amdgcn_alignbyte(rr[k + 1], rr[k], (unsigned)(od & 3));
    }
#pragma unroll
    for (int j = 0; j < 12; ++j) {
      const unsigned cc = byte_of(c, j + 3);
      unsigned lf = byte_of(c, j), rt = byte_of(c, j + 6);
      if (j < 3 && g == 0) lf = rt;                 // column 0: reflect-101
      if (j >= 9 && g == BB_G - 1) rt = lf;         // column 199
      const int l = (int)(lf + rt + byte_of(u, j) + byte_of(d, j)) - 4 * (int)cc;
      s_c[j % 3] += l;
      q_c[j % 3] += (unsigned)(l * l);
    }
  }

  long long acc[6];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) { acc[ch] = s_c[ch]; acc[3 + ch] = (long long)q_c[ch]; }
#pragma unroll
  for (int k = 0; k < 6; ++k)
    for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_down(acc[k], off, 64);
  if ((tid & 63) == 0)
    for (int k = 0; k < 6; ++k) red[tid >> 6][k] = (unsigned long long)acc[k];
  __syncthreads();
  if (tid == 0) {
    long long rec[8];
    rec[ST_FM_SY] = 0; rec[ST_FM_QY] = 0;
    for (int k = 0; k < 6; ++k) {
      unsigned long long t = 0;
      for (int wv = 0; wv < BB_T / 64; ++wv) t += red[wv][k];
      rec[ST_FM_S_R + k] = (long long)t;
    }
    if (bands > 1) {
      for (int k = 0; k < 6; ++k) part[(size_t)blockIdx.x * 6 + k] = (unsigned long long)rec[ST_FM_S_R + k];
      return;
    }
    if (out)
      for (int k = 0; k < 8; ++k) out[box * 8 + k] = (unsigned long long)rec[k];
    if (stat_out) fs_store(stat_out, box, kind, fs_value(rec, (long long)BB_S * BB_S, kind));
  }
}

// the banded launch's second half: one thread per box adds its bands' sums and writes the record and / or the statistic
__global__ __launch_bounds__(256) void k_bbox_finish(const unsigned long long* __restrict__ part, int bands, int m,
                                                     unsigned long long* __restrict__ out, int kind, void* stat_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  long long rec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int j = 0; j < bands; ++j)
    for (int k = 0; k < 6; ++k) rec[ST_FM_S_R + k] += (long long)part[((size_t)i * bands + j) * 6 + k];
  if (out)
    for (int k = 0; k < 8; ++k) out[(size_t)i * 8 + k] = (unsigned long long)rec[k];
  if (stat_out) fs_store(stat_out, (size_t)i, kind, fs_value(rec, (long long)BB_S * BB_S, kind));
}

// Rows per band: about four workgroups per CU over the call, at least 4 rows (halo rows are re-read), and few enough steps
// that no 32-bit per-lane partial can overflow: a lane adds at most 6 values per step to a group, each L^2 <= 1020^2, so
// 512 steps stay below 6 * 1020^2 * 512 < 2^32 (and Y^2 sums far below).
int fm_band_rows(st_ctx* ctx, int n, int h, int w) {
  const long long R = 3LL * w;
  const long long target = 4LL * ctx->num_cus;
  long long rows = ((long long)n * h + target - 1) / target;
  if (rows < 4) rows = 4;
  const long long max_rows = ((long long)(FM_MAX_STEPS - 2) * FM_STEP) / R;
  if (rows > max_rows) rows = max_rows;
  if (rows < 1) rows = 1;
  if (rows > h) rows = h;
  return (int)rows;
}

// smallest ring (log2 bytes) that holds 2 steps + 2 rows + slack; 0 if none fits
int fm_ring_log2(int what, int w) {
  const long long need = (what & ST_FM_LAPLACIAN) ? 2LL * FM_STEP + 2 * 3LL * w + 64 : 2LL * FM_STEP + 64;
  for (int lg = 15; lg <= FM_MAX_RING_LOG2; ++lg)
    if ((1LL << lg) >= need) return lg;
  return 0;
}

int fm_check(st_ctx* ctx, int n, int h, int w, int what, const void* out) {
  if (n < 0 || h <= 0 || w <= 0 || (what & ~(ST_FM_LUMA | ST_FM_LAPLACIAN)) || what == 0 || (n > 0 && !out))
    return st_set_error(ctx, ST_ERR_INVALID, "frame moments: bad arguments (n=%d h=%d w=%d what=%d)", n, h, w, what);
  if (3LL * h * w > 0x7fffffffLL)
    return st_set_error(ctx, ST_ERR_INVALID, "frame moments: %dx%d frames exceed 2^31 - 1 bytes", h, w);
  if (!fm_ring_log2(what, w) || 3LL * w > (long long)(FM_MAX_STEPS - 2) * FM_STEP)
    return st_set_error(ctx, ST_ERR_UNSUPPORTED, "frame moments: the Laplacian of rows wider than %d pixels is not implemented (w=%d)",
                        (int)(((1LL << FM_MAX_RING_LOG2) - 2LL * FM_STEP - 64) / 6), w);
  return ST_OK;
}

template <int WHAT>
void fm_launch_one(int lg, dim3 grid, hipStream_t s, hipEvent_t e0, hipEvent_t e1, FrameSrc src, int h, int w, int rows, unsigned long long* o) {
  if (lg == 15) hipExtLaunchKernelGGL((k_frame_moments<WHAT, 15>), grid, dim3(FM_T), 0, s, e0, e1, 0, src, h, w, rows, o);
  else if (lg == 16) hipExtLaunchKernelGGL((k_frame_moments<WHAT, 16>), grid, dim3(FM_T), 0, s, e0, e1, 0, src, h, w, rows, o);
  else hipExtLaunchKernelGGL((k_frame_moments<WHAT, 17>), grid, dim3(FM_T), 0, s, e0, e1, 0, src, h, w, rows, o);
}

int fm_launch(st_ctx* ctx, FrameSrc src, int n, int h, int w, int what, int64_t* out_dev) {
  ST_HIP(ctx, hipMemsetAsync(out_dev, 0, sizeof(int64_t) * 8 * (size_t)n, ctx->stream));
  const int rows = fm_band_rows(ctx, n, h, w);
  const int lg = fm_ring_log2(what, w);
  const unsigned bands = (unsigned)((h + rows - 1) / rows);
  return st_for_launches(n, [&](int f0, int nf) -> int {   // the frame index is grid.y
    FrameSrc s = src;
    if (s.ptrs) s.ptrs += f0; else s.base += (size_t)f0 * s.stride;
    unsigned long long* o = reinterpret_cast<unsigned long long*>(out_dev) + (size_t)f0 * 8;
    hipEvent_t e0, e1;
    ST_TRY(st_time_dispatch(ctx, ST_K_FRAME_STATS, &e0, &e1));
    const dim3 grid(bands, (unsigned)nf);
    if (what == ST_FM_LUMA) fm_launch_one<ST_FM_LUMA>(lg, grid, ctx->stream, e0, e1, s, h, w, rows, o);
    else if (what == ST_FM_LAPLACIAN) fm_launch_one<ST_FM_LAPLACIAN>(lg, grid, ctx->stream, e0, e1, s, h, w, rows, o);
    else fm_launch_one<ST_FM_LUMA | ST_FM_LAPLACIAN>(lg, grid, ctx->stream, e0, e1, s, h, w, rows, o);
    ST_HIP(ctx, hipGetLastError());
    return ST_OK;
  });
}

// Checks every box of a call and plans its resize; nothing has been enqueued when this fails
int bb_plan(st_ctx* ctx, int n, int h, int w, const int32_t* boxes_host, int64_t m, const void* out, std::vector<BoxK>* plan) {
  if (n < 0 || h <= 0 || w <= 0 || m < 0 || (m > 0 && (!boxes_host || !out)))
    return st_set_error(ctx, ST_ERR_INVALID, "bbox moments: bad arguments (n=%d h=%d w=%d m=%lld)", n, h, w, (long long)m);
  if (3LL * h * w > 0x7fffffffLL)
    return st_set_error(ctx, ST_ERR_INVALID, "bbox moments: %dx%d frames exceed 2^31 - 1 bytes", h, w);
  if (m > 0x7fffffffLL) return st_set_error(ctx, ST_ERR_UNSUPPORTED, "bbox moments: more than 2^31 - 1 boxes in one call");
  plan->resize((size_t)m);
  for (int64_t i = 0; i < m; ++i) {
    const int32_t* r = boxes_host + 5 * i;
    if (r[0] < 0 || r[0] >= n || r[1] < 0 || r[1] >= r[3] || r[3] > w || r[2] < 0 || r[2] >= r[4] || r[4] > h)
      return st_set_error(ctx, ST_ERR_INVALID, "bbox moments: box %lld {frame %d, x %d..%d, y %d..%d} is not inside one of %d frames of %dx%d",
                          (long long)i, r[0], r[1], r[3], r[2], r[4], n, w, h);
    BoxK& b = (*plan)[(size_t)i];
    b.frame = r[0]; b.x1 = r[1]; b.y1 = r[2]; b.bw = r[3] - r[1]; b.bh = r[4] - r[2];
    const st_rs_scales s = st_rs_plan_scales(b.bh, b.bw, BB_S, BB_S);
    b.mode = st_rs_linear_mode(b.bh, b.bw, BB_S, BB_S, s);
    b.scale_x = s.scale_x; b.scale_y = s.scale_y;
  }
  return ST_OK;
}

// frames_host: the caller's pointer table (uploaded here) or null for a strided stream
int bb_run(st_ctx* ctx, const uint8_t* const* frames_host, FrameSrc src, int n, int h, int w, const int32_t* boxes_host, int64_t m,
           int64_t* moments_dev, int kind, void* stat_dev) {
  std::vector<BoxK> plan;
  ST_TRY(bb_plan(ctx, n, h, w, boxes_host, m, moments_dev ? (const void*)moments_dev : stat_dev, &plan));
  if (m == 0) return ST_OK;
  // A workgroup fills one CU (its LDS) and a whole box keeps it busy for about 50 us: a call with fewer boxes than CUs cuts
  // every box into up to BB_MAX_BANDS bands of rows.  Integer sums: the record is the same bit for bit for any cut.
  int bands = (int)(ctx->num_cus / m);
  bands = bands < 1 ? 1 : (bands > BB_MAX_BANDS ? BB_MAX_BANDS : bands);
  const int band_rows = (BB_S + bands - 1) / bands;
  bands = (BB_S + band_rows - 1) / band_rows;
  const size_t bb = st_align_up(sizeof(BoxK) * (size_t)m);
  const size_t pb = bands > 1 ? st_align_up(sizeof(unsigned long long) * 6 * (size_t)m * bands) : 0;
  if (frames_host) {
    const uint8_t** table;
    ST_TRY(st_upload_tables(ctx, n, bb + pb, frames_host, &table));
    src.ptrs = table;
  } else {
    ST_TRY(st_ws_reserve(ctx, bb + pb));
  }
  BoxK* boxes = (BoxK*)st_ws_alloc(ctx, bb);
  unsigned long long* part = bands > 1 ? (unsigned long long*)st_ws_alloc(ctx, pb) : nullptr;
  if (!boxes || (bands > 1 && !part)) return st_set_error(ctx, ST_ERR_OOM, "bbox moments: scratch plan exhausted");
  // a pageable source: hipMemcpyAsync returns once the runtime has staged it, so the vector may go
  ST_HIP(ctx, hipMemcpyAsync(boxes, plan.data(), sizeof(BoxK) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
  hipEvent_t e0, e1;
  ST_TRY(st_time_dispatch(ctx, ST_K_FRAME_STATS, &e0, &e1));
  // boxes on grid.x, which reaches 2^31 - 1: one moments launch per call
  hipExtLaunchKernelGGL(k_bbox_moments, dim3((unsigned)(m * bands)), dim3(BB_T), 0, ctx->stream, e0, e1, 0, src, h, w, (const BoxK*)boxes,
                        bands, band_rows, part, reinterpret_cast<unsigned long long*>(moments_dev), kind, stat_dev);
  ST_HIP(ctx, hipGetLastError());
  if (bands > 1) {
    ST_TRY(st_time_dispatch(ctx, ST_K_FRAME_STATS, &e0, &e1));
    hipExtLaunchKernelGGL(k_bbox_finish, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, e0, e1, 0,
                          (const unsigned long long*)part, bands, (int)m, reinterpret_cast<unsigned long long*>(moments_dev), kind, stat_dev);
    ST_HIP(ctx, hipGetLastError());
  }
  return ST_OK;
}

int bb_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, const int32_t* boxes_host, int64_t m, int64_t* moments_dev,
             int kind, void* stat_dev) {
  ST_TRY(st_enter(ctx));
  if (n > 0 && m > 0) {
    if (!frames_dev) return st_set_error(ctx, ST_ERR_INVALID, "bbox moments: null frame table");
    ST_TRY(st_check_rows(ctx, "bbox moments: frame %d is null", n, false, frames_dev));
  }
  return bb_run(ctx, frames_dev, FrameSrc{nullptr, nullptr, 0}, n, h, w, boxes_host, m, moments_dev, kind, stat_dev);
}

int bb_strided(st_ctx* ctx, const uint8_t* base_dev, size_t stride, int n, int h, int w, const int32_t* boxes_host, int64_t m,
               int64_t* moments_dev, int kind, void* stat_dev) {
  ST_TRY(st_enter(ctx));
  if (n > 0 && m > 0 && h > 0 && w > 0 && (!base_dev || stride < (size_t)3 * h * w))
    return st_set_error(ctx, ST_ERR_INVALID, "bbox moments: bad base/stride");
  return bb_run(ctx, nullptr, FrameSrc{nullptr, base_dev, stride}, n, h, w, boxes_host, m, moments_dev, kind, stat_dev);
}

int bb_kind_check(st_ctx* ctx, int kind) {
  ST_TRY(st_enter(ctx));
  if (kind != ST_FS_SHARPNESS_CPP && kind != ST_FS_SHARPNESS)
    return st_set_error(ctx, ST_ERR_INVALID, "bbox sharpness: kind %d is neither ST_FS_SHARPNESS_CPP nor ST_FS_SHARPNESS", kind);
  return ST_OK;
}

}  // namespace

ST_EXPORT int st_frame_moments_u8c3_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int what,
                                          int64_t* moments_dev) {
  ST_TRY(st_enter(ctx));
  ST_TRY(fm_check(ctx, n, h, w, what, moments_dev));
  if (n == 0) return ST_OK;
  if (!frames_dev) return st_set_error(ctx, ST_ERR_INVALID, "frame moments: null frame table");
  ST_TRY(st_check_rows(ctx, "frame moments: frame %d is null", n, false, frames_dev));
  const uint8_t** table;
  ST_TRY(st_upload_tables(ctx, n, 0, frames_dev, &table));
  return fm_launch(ctx, FrameSrc{table, nullptr, 0}, n, h, w, what, moments_dev);
}

ST_EXPORT int st_frame_moments_u8c3_strided(st_ctx* ctx, const uint8_t* base_dev, size_t frame_stride_bytes, int n, int h, int w,
                                            int what, int64_t* moments_dev) {
  ST_TRY(st_enter(ctx));
  ST_TRY(fm_check(ctx, n, h, w, what, moments_dev));
  if (n == 0) return ST_OK;
  if (!base_dev || frame_stride_bytes < (size_t)3 * h * w) return st_set_error(ctx, ST_ERR_INVALID, "frame moments: bad base/stride");
  return fm_launch(ctx, FrameSrc{nullptr, base_dev, frame_stride_bytes}, n, h, w, what, moments_dev);
}

ST_EXPORT int st_frame_stats_finish(st_ctx* ctx, const int64_t* moments_dev, int n, int h, int w, int kind, void* out_dev) {
  ST_TRY(st_enter(ctx));
  if (n < 0 || h <= 0 || w <= 0 || kind < 0 || kind > ST_FS_SHARPNESS || (n > 0 && (!moments_dev || !out_dev)) ||
      3LL * h * w > 0x7fffffffLL)
    return st_set_error(ctx, ST_ERR_INVALID, "frame stats: bad arguments (n=%d h=%d w=%d kind=%d)", n, h, w, kind);
  if (n == 0) return ST_OK;
  hipEvent_t e0, e1;
  ST_TRY(st_time_dispatch(ctx, ST_K_FRAME_STATS, &e0, &e1));
  hipExtLaunchKernelGGL(k_frame_stats_finish, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, e0, e1, 0, (const long long*)moments_dev, n,
                        (long long)h * w, kind, out_dev);
  ST_HIP(ctx, hipGetLastError());
  return ST_OK;
}

ST_EXPORT int st_bbox_moments_u8c3_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, const int32_t* boxes_host,
                                         int64_t m, int64_t* moments_dev) {
  return bb_batch(ctx, frames_dev, n, h, w, boxes_host, m, moments_dev, 0, nullptr);
}

ST_EXPORT int st_bbox_moments_u8c3_strided(st_ctx* ctx, const uint8_t* base_dev, size_t frame_stride_bytes, int n, int h, int w,
                                           const int32_t* boxes_host, int64_t m, int64_t* moments_dev) {
  return bb_strided(ctx, base_dev, frame_stride_bytes, n, h, w, boxes_host, m, moments_dev, 0, nullptr);
}

ST_EXPORT int st_bbox_sharpness_u8c3_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, const int32_t* boxes_host,
                                           int64_t m, int kind, void* out_dev) {
  ST_TRY(bb_kind_check(ctx, kind));
  return bb_batch(ctx, frames_dev, n, h, w, boxes_host, m, nullptr, kind, out_dev);
}

ST_EXPORT int st_bbox_sharpness_u8c3_strided(st_ctx* ctx, const uint8_t* base_dev, size_t frame_stride_bytes, int n, int h, int w,
                                             const int32_t* boxes_host, int64_t m, int kind, void* out_dev) {
  ST_TRY(bb_kind_check(ctx, kind));
  return bb_strided(ctx, base_dev, frame_stride_bytes, n, h, w, boxes_host, m, nullptr, kind, out_dev);
}
