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

__global__ __launch_bounds__(256) void k_frame_stats_finish(const long long* __restrict__ m, int n, long long N, int kind, void* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long* r = m + (size_t)i * 8;
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
  if (kind <= ST_FS_SHARPNESS_CPP) reinterpret_cast<float*>(out)[i] = (float)v;
  else reinterpret_cast<double*>(out)[i] = v;
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
  // grid.y is limited to 65535 frames per launch
  for (int f0 = 0; f0 < n; f0 += 65535) {
    const int nf = n - f0 < 65535 ? n - f0 : 65535;
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
  }
  return ST_OK;
}

}  // namespace

ST_EXPORT int st_frame_moments_u8c3_batch(st_ctx* ctx, const uint8_t* const* frames_dev, int n, int h, int w, int what,
                                          int64_t* moments_dev) {
  ST_TRY(st_enter(ctx));
  ST_TRY(fm_check(ctx, n, h, w, what, moments_dev));
  if (n == 0) return ST_OK;
  if (!frames_dev) return st_set_error(ctx, ST_ERR_INVALID, "frame moments: null frame table");
  for (int i = 0; i < n; ++i)
    if (!frames_dev[i]) return st_set_error(ctx, ST_ERR_INVALID, "frame moments: frame %d is null", i);
  ST_TRY(st_ws_reserve(ctx, st_align_up(sizeof(void*) * (size_t)n)));
  const uint8_t** table = (const uint8_t**)st_ws_alloc(ctx, sizeof(void*) * (size_t)n);
  ST_HIP(ctx, hipMemcpyAsync(table, frames_dev, sizeof(void*) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
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
