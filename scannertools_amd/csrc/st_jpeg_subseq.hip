// ImageDecoder op, entropy stage on the device by SUBSEQUENCE: the kernels of st_jpeg_decode_batch_gpu_split (st_jpeg.hip has the
// call and the upload; st_jpeg_entropy.h the bounded core they run, which the host runs in st_jpeg_coefficients_by_subsequence;
// DESIGN.md 4.12 the contract).  Streams need no restart intervals: a segment (a restart interval, or the whole scan) is cut into
// subsequences of S raw bytes and a lane is one subsequence.
//
//   k_jsq_round     F_i(e_{i-1}) for every lane, up to 16 rounds per launch inside a workgroup: a workgroup is 64 consecutive
//                   lanes of ONE frame (they may span segments), the frame's tables, geometry and zigzag order staged in LDS as
//                   k_jpeg_entropy_dec stages them, the 64 exit states in LDS with a barrier per round.  Its first lane enters
//                   from the exit its predecessor had when the PREVIOUS launch ended (the exit states ping-pong between two
//                   arrays), so no workgroup ever waits on another: a stale predecessor costs a launch, never a hang.  A lane
//                   whose entering state is the one it last decoded from skips the round.  Each launch counts the exits it
//                   changed; a launch that changes none has verified the chain.
//   k_jsq_scan      one wave per segment, looping over the segment's lanes 64 at a time with a carry: the exclusive prefix of
//                   (blocks, DC sums per component), whether the chain is intact in front of each lane, and whether every lane
//                   entered from its predecessor's exit -- if not (the rounds were capped), the segment is marked unconverged.
//   k_jsq_zero      the sub-batch's coefficients, zeroed: a block may be filled by two lanes, so no lane may zero it.
//   k_jsq_write     every lane of a converged segment walks its subsequence once more from its entering state and stores absolute
//                   DC values and AC coefficients; a lane on the intact chain that fails folds (stream, segment, cause) into the
//                   status word.
//   k_jsq_fallback  one lane per unconverged segment: st_jpeg_decode_interval, slow and always exact.
// Ordering between workgroups comes from the launch boundaries alone.  grid.x strides over the frames and grid.y over a frame's
// groups of 64 lanes (or its segments), so neither count is bounded by a grid dimension.
#include "st_internal.h"
#include "st_jpeg_entropy.h"

namespace {

constexpr int kHuffWords = (int)(sizeof(StJpegHuff) / 4);
static_assert(sizeof(StJpegHuff) % 4 == 0 && sizeof(StJpegFrameTables) == 6 * sizeof(StJpegHuff), "tables are copied as dwords");
static_assert(sizeof(StJpegScanGeom) == 64, "the geometry is 16 dwords");

// the frame's tables and geometry into LDS; the caller's barrier follows
__device__ __forceinline__ void stage_frame(const StJpegEntArgs& a, const StJpegEntFrame* __restrict__ fr, StJpegFrameTables* tabs, StJpegScanGeom* geom, int lane) {
  const int ncomp = fr->geom.ncomp < 3 ? 1 : 3;
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(a.tables + fr->tables);
  uint32_t* dst = reinterpret_cast<uint32_t*>(tabs);
  for (int i = lane; i < ncomp * kHuffWords; i += kStJsqLanes) {
    dst[i] = src[i];                                     // dc[0 .. ncomp)
    dst[3 * kHuffWords + i] = src[3 * kHuffWords + i];   // ac[0 .. ncomp)
  }
  if (lane < 16) reinterpret_cast<int32_t*>(geom)[lane] = reinterpret_cast<const int32_t*>(&fr->geom)[lane];
}

// What a lane is: subsequence `j` of segment `k` of its frame.
struct LaneAt {
  uint32_t k, j, nsub;
  uint32_t seg_begin, seg_end;   // bytes of the segment, relative to the frame's first entropy-coded byte, clipped to it
  uint32_t sub_begin, sub_end;
};

// lane `li` (< the frame's lanes) from the frame's prefix table of subsequence counts: the last segment whose prefix is <= li
__device__ __forceinline__ LaneAt lane_at(const StJsqArgs& a, const StJpegEntFrame* __restrict__ fr, const StJsqFrame* __restrict__ sq, uint32_t li) {
  const uint32_t* __restrict__ pre = reinterpret_cast<const uint32_t*>(a.ent.upload + sq->subpre_off);
  const uint32_t* __restrict__ iv = reinterpret_cast<const uint32_t*>(a.ent.upload + fr->intervals_off);
  uint32_t lo = 0, hi = fr->nint;   // pre[lo] <= li < pre[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (pre[mid] <= li) lo = mid; else hi = mid;
  }
  LaneAt at;
  at.k = lo;
  at.j = li - pre[lo];
  at.nsub = pre[lo + 1] - pre[lo];
  const uint32_t nbytes = fr->nbytes;
  const uint32_t b = iv[2 * lo], e = iv[2 * lo + 1];
  at.seg_begin = b < nbytes ? b : nbytes;
  at.seg_end = e < nbytes ? e : nbytes;
  if (at.seg_end < at.seg_begin) at.seg_end = at.seg_begin;
  const uint64_t sb = (uint64_t)at.seg_begin + (uint64_t)at.j * a.S, se = sb + a.S;
  at.sub_begin = sb < at.seg_end ? (uint32_t)sb : at.seg_end;
  at.sub_end = se < at.seg_end ? (uint32_t)se : at.seg_end;
  return at;
}

// the segment's first MCU and the blocks it holds, clipped to the frame
__device__ __forceinline__ void segment_blocks(const StJpegScanGeom& g, uint32_t k, long long* mcu0, uint32_t* seg_blocks, int* nmcu) {
  const long long total = (long long)g.mcux * g.mcuy;
  const int ri = g.restart_interval;
  *mcu0 = ri > 0 ? (long long)k * ri : 0;
  long long n = ri > 0 ? (ri < total - *mcu0 ? ri : total - *mcu0) : total;
  if (n < 0) n = 0;
  *nmcu = (int)(n < 0x7fffffff ? n : 0x7fffffff);
  *seg_blocks = (uint32_t)(n * st_jsq_mcu_blocks(g));
}

__global__ __launch_bounds__(kStJsqLanes) void k_jsq_round(StJsqArgs a, int first, int par, int rounds, unsigned* changed) {
  __shared__ StJpegFrameTables tabs;
  __shared__ StJpegScanGeom geom;
  __shared__ uint8_t zz[64];
  __shared__ uint64_t s_exit[kStJsqLanes];
  const int lane = threadIdx.x;
  zz[lane] = (uint8_t)st_jpeg_natural(lane);   // read after the barrier every frame's staging ends with
  const uint64_t* __restrict__ ein = a.exits[par ^ 1];
  uint64_t* __restrict__ eout = a.exits[par];
  unsigned nchanged = 0;
  for (int f = blockIdx.x; f < a.ent.nf; f += gridDim.x) {
    const StJpegEntFrame* __restrict__ fr = a.ent.frames + f;
    const StJsqFrame* __restrict__ sq = a.sq + f;
    const uint32_t nlanes = sq->nlanes;
    const uint32_t ngroups = (nlanes + kStJsqLanes - 1) / kStJsqLanes;
    if (blockIdx.y >= ngroups) continue;   // uniform over the workgroup
    __syncthreads();                       // the previous frame's lanes are done with the tables
    stage_frame(a.ent, fr, &tabs, &geom, lane);
    __syncthreads();
    const uint8_t* __restrict__ bytes = a.ent.upload + fr->bytes_off;
    for (uint32_t g = blockIdx.y; g < ngroups; g += gridDim.y) {
      const uint32_t li = g * kStJsqLanes + (uint32_t)lane;
      const bool active = li < nlanes;
      LaneAt at = {};
      if (active) at = lane_at(a, fr, sq, li);
      const size_t G = (size_t)sq->lane_off + li;
      const bool starts = at.j == 0;   // the first lane of a segment enters from the segment's true start
      uint64_t e = kStJsqInvalid, from = kStJsqNever, left = kStJsqInvalid;
      if (active && !first) {
        e = ein[G];
        from = a.entered[G];
        if (lane == 0 && !starts) left = ein[G - 1];   // as the previous launch left it
      }
      __syncthreads();   // the previous group's rounds are over
      s_exit[lane] = e;
      for (int r = 0; r < rounds; ++r) {
        __syncthreads();
        const uint64_t enter = starts ? st_jsq_pack(at.seg_begin, 0, 0, 0) : (lane == 0 ? left : s_exit[lane - 1]);
        int ch = 0;
        if (active && enter != from) {
          const uint64_t go = enter == kStJsqInvalid ? st_jsq_guess(bytes, at.seg_begin, at.seg_end, at.sub_begin) : enter;
          StJsqOut o;
          st_jsq_run<false, true>(bytes, at.seg_end, at.sub_end, false, go, geom, &tabs, zz, 0, 0, 0, nullptr, nullptr, &o);
          *reinterpret_cast<uint4*>(a.counts + 4 * G) = make_uint4(o.blocks, o.dc[0], o.dc[1], o.dc[2]);
          from = enter;
          ch = o.exit != e;
          e = o.exit;
          nchanged += (unsigned)ch;
        }
        __syncthreads();   // every lane has read its neighbour's exit
        s_exit[lane] = e;
        if (!__syncthreads_or(ch)) break;   // no exit of the group changed: its next round would change none
      }
      if (active) {
        eout[G] = e;
        a.entered[G] = from;
      }
    }
  }
  if (nchanged) atomicAdd(changed, nchanged);
}

// One wave per segment.  After it: counts[lane] is the exclusive prefix over the segment, entered[lane] the state the write step
// enters with, or kStJsqInvalid where an exit in front of the lane is invalid.
__global__ __launch_bounds__(kStJsqLanes) void k_jsq_scan(StJsqArgs a, int par) {
  const int lane = threadIdx.x;
  const uint64_t* __restrict__ exits = a.exits[par];
  for (int f = blockIdx.x; f < a.ent.nf; f += gridDim.x) {
    const StJpegEntFrame* __restrict__ fr = a.ent.frames + f;
    const StJsqFrame* __restrict__ sq = a.sq + f;
    const uint32_t* __restrict__ pre = reinterpret_cast<const uint32_t*>(a.ent.upload + sq->subpre_off);
    const uint32_t* __restrict__ iv = reinterpret_cast<const uint32_t*>(a.ent.upload + fr->intervals_off);
    const uint32_t nseg = fr->nint, nbytes = fr->nbytes;
    for (uint32_t k = blockIdx.y; k < nseg; k += gridDim.y) {
      const uint32_t nsub = pre[k + 1] - pre[k];
      const size_t G0 = (size_t)sq->lane_off + pre[k];
      const uint32_t b0 = iv[2 * k];
      const uint64_t start = st_jsq_pack(b0 < nbytes ? b0 : nbytes, 0, 0, 0);
      uint32_t carry[4] = {0, 0, 0, 0};
      bool intact = true, stale = false;
      for (uint32_t base = 0; base < nsub; base += kStJsqLanes) {
        const uint32_t j = base + (uint32_t)lane;
        const bool active = j < nsub;
        uint4 c = make_uint4(0, 0, 0, 0);
        uint64_t e = kStJsqInvalid, from = kStJsqNever, left = start;
        if (active) {
          c = *reinterpret_cast<const uint4*>(a.counts + 4 * (G0 + j));
          e = exits[G0 + j];
          from = a.entered[G0 + j];
          if (j > 0) left = exits[G0 + j - 1];
        }
        // a lane that did not enter from its predecessor's exit: the rounds were capped before the chain was verified
        if (__ballot(active && from != left) != 0ull) stale = true;
        // intact in front of lane t: no invalid exit among the lanes before it
        const unsigned long long bad = __ballot(active && e == kStJsqInvalid);
        const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
        const bool ok = intact && (bad & below) == 0ull;
        // inclusive prefix over the wave, then exclusive with the carry
        uint32_t v[4] = {c.x, c.y, c.z, c.w}, inc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          uint32_t s = v[q];
#pragma unroll
          for (int d = 1; d < kStJsqLanes; d <<= 1) {
            const uint32_t up = __shfl_up(s, d, kStJsqLanes);
            if (lane >= d) s += up;
          }
          inc[q] = s;
        }
        if (active) {
          *reinterpret_cast<uint4*>(a.counts + 4 * (G0 + j)) =
              make_uint4(carry[0] + inc[0] - v[0], carry[1] + inc[1] - v[1], carry[2] + inc[2] - v[2], carry[3] + inc[3] - v[3]);
          a.entered[G0 + j] = ok ? from : kStJsqInvalid;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) carry[q] += __shfl(inc[q], kStJsqLanes - 1, kStJsqLanes);
        if (bad != 0ull) intact = false;
      }
      if (lane == 0) a.unconverged[sq->seg_off + k] = stale ? 1u : 0u;
    }
  }
}

__global__ __launch_bounds__(256) void k_jsq_zero(uint4* __restrict__ p, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(kStJsqLanes) void k_jsq_write(StJsqArgs a) {
  __shared__ StJpegFrameTables tabs;
  __shared__ StJpegScanGeom geom;
  __shared__ uint8_t zz[64];
  const int lane = threadIdx.x;
  zz[lane] = (uint8_t)st_jpeg_natural(lane);
  for (int f = blockIdx.x; f < a.ent.nf; f += gridDim.x) {
    const StJpegEntFrame* __restrict__ fr = a.ent.frames + f;
    const StJsqFrame* __restrict__ sq = a.sq + f;
    const uint32_t nlanes = sq->nlanes;
    const uint32_t ngroups = (nlanes + kStJsqLanes - 1) / kStJsqLanes;
    if (blockIdx.y >= ngroups) continue;
    __syncthreads();
    stage_frame(a.ent, fr, &tabs, &geom, lane);
    __syncthreads();
    const uint8_t* __restrict__ bytes = a.ent.upload + fr->bytes_off;
    int16_t* coef = a.ent.coef + (size_t)fr->blk_off * 64;
    for (uint32_t g = blockIdx.y; g < ngroups; g += gridDim.y) {
      const uint32_t li = g * kStJsqLanes + (uint32_t)lane;
      if (li >= nlanes) continue;   // no barrier below
      const LaneAt at = lane_at(a, fr, sq, li);
      if (a.unconverged[sq->seg_off + at.k]) continue;   // k_jsq_fallback decodes the segment
      const size_t G = (size_t)sq->lane_off + li;
      const uint64_t enter = a.entered[G];
      if (enter == kStJsqInvalid) continue;   // the chain is broken in front of the lane: the lane that broke it reports
      const uint4 c = *reinterpret_cast<const uint4*>(a.counts + 4 * G);
      long long mcu0;
      uint32_t seg_blocks;
      int nmcu;
      segment_blocks(geom, at.k, &mcu0, &seg_blocks, &nmcu);
      if (c.x >= seg_blocks) continue;        // behind the segment's last block: stray bytes, decoded by nobody
      const uint32_t dc[3] = {c.y, c.z, c.w};
      StJsqOut o;
      const int st = st_jsq_run<true, true>(bytes, at.seg_end, at.sub_end, at.j + 1 == at.nsub, enter, geom, &tabs, zz, mcu0, seg_blocks, c.x, dc, coef, &o);
      if (st != ST_JE_OK)
        atomicMin(a.ent.status, ((unsigned long long)(unsigned)(a.ent.first_stream + f) << 32) | ((unsigned long long)at.k << 4) | (unsigned long long)st);
    }
  }
}

__global__ __launch_bounds__(kStJsqLanes) void k_jsq_fallback(StJsqArgs a) {
  __shared__ StJpegFrameTables tabs;
  __shared__ StJpegScanGeom geom;
  __shared__ uint8_t zz[64];
  const int lane = threadIdx.x;
  zz[lane] = (uint8_t)st_jpeg_natural(lane);
  for (int f = blockIdx.x; f < a.ent.nf; f += gridDim.x) {
    const StJpegEntFrame* __restrict__ fr = a.ent.frames + f;
    const StJsqFrame* __restrict__ sq = a.sq + f;
    const uint32_t nseg = fr->nint;
    const uint32_t ngroups = (nseg + kStJsqLanes - 1) / kStJsqLanes;
    if (blockIdx.y >= ngroups) continue;
    // the tables are staged only where a segment of the frame needs them (uniform: a barrier inside)
    bool any = false;
    for (uint32_t g = blockIdx.y; g < ngroups; g += gridDim.y) {
      const uint32_t k = g * kStJsqLanes + (uint32_t)lane;
      any = any || (k < nseg && a.unconverged[sq->seg_off + k] != 0);
    }
    if (!__syncthreads_or(any)) continue;
    stage_frame(a.ent, fr, &tabs, &geom, lane);
    __syncthreads();
    const uint32_t* __restrict__ iv = reinterpret_cast<const uint32_t*>(a.ent.upload + fr->intervals_off);
    const uint8_t* __restrict__ bytes = a.ent.upload + fr->bytes_off;
    const uint32_t nbytes = fr->nbytes;
    int16_t* coef = a.ent.coef + (size_t)fr->blk_off * 64;
    for (uint32_t g = blockIdx.y; g < ngroups; g += gridDim.y) {
      const uint32_t k = g * kStJsqLanes + (uint32_t)lane;
      if (k >= nseg || !a.unconverged[sq->seg_off + k]) continue;
      long long mcu0;
      uint32_t seg_blocks;
      int nmcu;
      segment_blocks(geom, k, &mcu0, &seg_blocks, &nmcu);
      const uint32_t begin = iv[2 * k], end = iv[2 * k + 1];
      const int st = st_jpeg_decode_interval<true>(bytes, begin < nbytes ? begin : nbytes, end < nbytes ? end : nbytes, mcu0, nmcu, geom, &tabs, zz, coef);
      if (st != ST_JE_OK)
        atomicMin(a.ent.status, ((unsigned long long)(unsigned)(a.ent.first_stream + f) << 32) | ((unsigned long long)k << 4) | (unsigned long long)st);
    }
  }
}

dim3 lane_grid(int nf, unsigned max_groups) {
  unsigned gy = max_groups < 1024u ? (max_groups ? max_groups : 1u) : 1024u;
  unsigned gx = nf < (1 << 20) ? (unsigned)nf : (1u << 20);
  if ((unsigned long long)gx * gy > (1ull << 24)) gx = (1u << 24) / gy;
  return dim3(gx, gy);
}

}  // namespace

int st_jsq_round_launch(st_ctx* ctx, const StJsqArgs& a, unsigned max_groups, bool first, int par, unsigned* changed) {
  if (a.ent.nf <= 0) return ST_OK;
  hipLaunchKernelGGL(k_jsq_round, lane_grid(a.ent.nf, max_groups), dim3(kStJsqLanes), 0, ctx->stream, a, first ? 1 : 0, par, kStJsqRoundsPerLaunch, changed);
  ST_HIP(ctx, hipGetLastError());
  return ST_OK;
}

int st_jsq_finish_launch(st_ctx* ctx, const StJsqArgs& a, unsigned max_groups, unsigned max_segments, int par, size_t coef_bytes) {
  if (a.ent.nf <= 0) return ST_OK;
  hipLaunchKernelGGL(k_jsq_scan, lane_grid(a.ent.nf, max_segments), dim3(kStJsqLanes), 0, ctx->stream, a, par);
  const size_t n16 = coef_bytes / 16;   // a block is 128 bytes and the coefficients start 16-byte aligned
  size_t zb = (n16 + 255) / 256;
  if (zb > 16384) zb = 16384;
  if (zb) hipLaunchKernelGGL(k_jsq_zero, dim3((unsigned)zb), dim3(256), 0, ctx->stream, reinterpret_cast<uint4*>(a.ent.coef), n16);
  hipLaunchKernelGGL(k_jsq_write, lane_grid(a.ent.nf, max_groups), dim3(kStJsqLanes), 0, ctx->stream, a);
  hipLaunchKernelGGL(k_jsq_fallback, lane_grid(a.ent.nf, (max_segments + kStJsqLanes - 1) / kStJsqLanes), dim3(kStJsqLanes), 0, ctx->stream, a);
  ST_HIP(ctx, hipGetLastError());
  return ST_OK;
}
