// ImageDecoder op, entropy stage on the device: k_jpeg_entropy_dec, the Huffman decoder of st_jpeg_decode_batch_gpu (st_jpeg.hip
// has the call, the upload layout and the two dense kernels that follow).
//
// One lane per restart interval, running st_jpeg_decode_interval (st_jpeg_entropy.h) -- the same bounded core the host runs in
// st_jpeg_coefficients_by_interval.  A workgroup is one wave of 64 lanes = 64 consecutive intervals of ONE frame; the frame's
// geometry and Huffman tables are staged in LDS once per workgroup (two tables per component: 2.8 KB for a one-component
// frame, 8.4 KB for three; the zigzag order beside them), so the table walks are LDS reads and only stream bytes and coefficients touch memory.  The stream
// bytes come in aligned 8-byte words requested two words ahead (the upload aligns every stream to 16 bytes and pads it by 16):
// an eighth of the load instructions of a bytewise reader.  The launch's time is one lane's walk through its interval
// (DESIGN.md 4.12 has the measurement), the same with either reader at up to 256 1080p frames.  Each lane
// zeroes each of its blocks before it fills it (the core does, as the host decoder does): no memset precedes the launch.
// grid.x strides over the frames and grid.y over a frame's interval groups, so neither count is bounded by a grid dimension.
// A lane whose interval is corrupt stops and folds (stream, interval, cause) into the status word with one atomic minimum.
#include "st_internal.h"
#include "st_jpeg_entropy.h"

namespace {

constexpr int kHuffWords = (int)(sizeof(StJpegHuff) / 4);
static_assert(sizeof(StJpegHuff) % 4 == 0 && sizeof(StJpegFrameTables) == 6 * sizeof(StJpegHuff), "tables are copied as dwords");
static_assert(sizeof(StJpegScanGeom) == 64, "the geometry is 16 dwords");

__global__ __launch_bounds__(kStJpegEntLanes) void k_jpeg_entropy_dec(StJpegEntArgs a) {
  __shared__ StJpegFrameTables tabs;
  __shared__ StJpegScanGeom geom;
  __shared__ uint8_t zz[64];
  const int lane = threadIdx.x;
  zz[lane] = (uint8_t)st_jpeg_natural(lane);   // read after the barrier every frame's staging ends with
  for (int f = blockIdx.x; f < a.nf; f += gridDim.x) {
    const StJpegEntFrame* __restrict__ fr = a.frames + f;
    const unsigned nint = fr->nint;
    const unsigned ngroups = (nint + kStJpegEntLanes - 1) / kStJpegEntLanes;
    if (blockIdx.y >= ngroups) continue;   // uniform over the workgroup
    __syncthreads();                       // the previous frame's lanes are done with the tables
    {
      const int ncomp = fr->geom.ncomp < 3 ? 1 : 3;
      const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(a.tables + fr->tables);
      uint32_t* dst = reinterpret_cast<uint32_t*>(&tabs);
      for (int i = lane; i < ncomp * kHuffWords; i += kStJpegEntLanes) {
        dst[i] = src[i];                                     // dc[0 .. ncomp)
        dst[3 * kHuffWords + i] = src[3 * kHuffWords + i];   // ac[0 .. ncomp)
      }
      if (lane < 16) reinterpret_cast<int32_t*>(&geom)[lane] = reinterpret_cast<const int32_t*>(&fr->geom)[lane];
    }
    __syncthreads();
    const int ri = geom.restart_interval;
    const uint32_t* __restrict__ iv = reinterpret_cast<const uint32_t*>(a.upload + fr->intervals_off);
    const uint8_t* __restrict__ bytes = a.upload + fr->bytes_off;
    const uint32_t nbytes = fr->nbytes;
    int16_t* coef = a.coef + (size_t)fr->blk_off * 64;
    for (unsigned g = blockIdx.y; g < ngroups; g += gridDim.y) {
      const unsigned k = g * kStJpegEntLanes + (unsigned)lane;
      if (k >= nint) continue;
      const uint32_t begin = iv[2 * k], end = iv[2 * k + 1];
      const int st = st_jpeg_decode_interval<true>(bytes, begin < nbytes ? begin : nbytes, end < nbytes ? end : nbytes, (long long)k * ri, ri, geom, &tabs, zz, coef);
      if (st != ST_JE_OK)
        atomicMin(a.status, ((unsigned long long)(unsigned)(a.first_stream + f) << 32) | ((unsigned long long)k << 4) | (unsigned long long)st);
    }
  }
}

}  // namespace

int st_jpeg_entropy_launch(st_ctx* ctx, const StJpegEntArgs& a, unsigned max_groups) {
  if (a.nf <= 0 || max_groups == 0) return ST_OK;
  unsigned gy = max_groups < 1024u ? max_groups : 1024u;
  unsigned gx = a.nf < (1 << 20) ? (unsigned)a.nf : (1u << 20);
  if ((unsigned long long)gx * gy > (1ull << 24)) gx = (1u << 24) / gy;
  hipLaunchKernelGGL(k_jpeg_entropy_dec, dim3(gx, gy), dim3(kStJpegEntLanes), 0, ctx->stream, a);
  ST_HIP(ctx, hipGetLastError());
  return ST_OK;
}
