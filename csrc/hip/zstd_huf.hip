// GPU decode of Huffman-only zstd pages (gfx950): one 256-thread workgroup
// per Huffman stream (four per page, one for a single-stream page), the
// stream cut into 256 sub-sequences decoded at once (csrc/cpp/huf_par.h,
// which holds the per-lane steps; the host twin there runs the same code).
//
// A Huffman-only page (lszstd::huf_only_frame) is one compressed block
// with a tree description, 1 or 4 streams and no sequences: float columns
// and wide-range integers compress to exactly this. zstd_pages_kernel
// gives such a page 4 busy lanes, each walking ~32 K symbols through a
// dependent LDS lookup; here 1024 lanes walk ~125 symbols each a few times.
//
// Why a workgroup per stream and not a wave per stream: a scan unit holds
// only about 290 such pages, and the chain per lane is latency-bound (LDS
// lookup, then shift, then the next lookup). With one workgroup per page
// and 64 lanes per stream the unit occupied one wave per SIMD on 256 CUs
// and took 0.84 ms; with four times the lanes it takes 0.41 ms
// (profiles/r03_gpu_huf.md).
//
// - the tree description (at most 128 bytes) is staged in LDS, where
//   thread 0 builds the decode table with the shared read_huf_tree: its
//   bit-by-bit forward reader would otherwise wait on global memory for
//   every bit. Each of a page's workgroups builds the table for itself.
//   (Staging the stream's bytes in LDS as well, for the lanes' window
//   refills, was measured slower: 0.54 against 0.41 ms per unit.)
// - pass 1, then fix-up rounds: exits go through LDS, a round ends at a
//   workgroup-wide "did any lane change";
// - counts are prefix-summed (wave shuffles, wave totals through LDS); the
//   stream is valid only if they sum to its expected length and the last
//   lane exits on the stream's first bit. Then the write pass stores
//   straight into dst, packed into aligned 8-byte stores with a byte head
//   and tail. No scratch buffer, no copy.
// - status[page] is zeroed by the caller; a workgroup that refuses its
//   stream stores 1 and writes nothing. The other streams of such a page
//   may have written their own slices of the page's output range.
//
// Table layout: HufEntry is 2 bytes, so the table spans 2^maxBits / 2
// consecutive dwords and the lanes' lookups are divergent ds_read_u8 /
// ds_read_u16 over 32 banks: a few-way conflict per lookup on near-random
// bytes. The lookup chain is latency-bound, and with every CU filled the
// kernel is bound by the VALU work per symbol (window shift, mask, compare:
// about 20 instructions), not by LDS throughput, so the layout stays the
// one shared with the host.

#include <hip/hip_runtime.h>

#include "../cpp/huf_par.h"
#include "kernels.h"

namespace lsz_gpu {

using namespace lszstd;

static const int kHufLanes = 256;  // threads per workgroup = lanes per stream
static const int kHufWaves = kHufLanes / 64;
static const int kHufDescMax = 128;  // 1 + 127 FSE bytes, or 1 + 64 nibbles

struct HufLds {
  HufTable huf;
  BuildWs ws;                   // thread 0's table-build workspace
  uint8_t desc[kHufDescMax];    // the tree description's bytes
  int32_t exitb[kHufLanes];     // where each lane left, for its successor
  int32_t wsum[kHufWaves];      // per-wave count totals
  int64_t used;                 // bytes of the tree description, -1: bad
};

// wave-inclusive prefix sum
__device__ inline int32_t wave_scan(int32_t v, int wlane) {
  for (int d = 1; d < 64; d <<= 1) {
    int32_t u = __shfl_up(v, d);
    if (wlane >= d) v += u;
  }
  return v;
}

__global__ void __launch_bounds__(kHufLanes) zstd_huf_pages_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ jobs,
    int64_t njobs, uint8_t* __restrict__ dst, int32_t* __restrict__ status) {
  __shared__ HufLds c;
  const int lane = threadIdx.x;
  // work item = (page, stream); everything up to the fix-up loop depends
  // on the item alone, so every branch that leaves is workgroup-uniform
  for (int64_t item = blockIdx.x; item < 4 * njobs; item += gridDim.x) {
    const int64_t pg = item >> 2;
    const int stream = (int)(item & 3);
    const int64_t* j = jobs + 4 * pg;
    const uint8_t* frame = src + j[0];
    const int64_t rs = j[3];
    HufOnly ho;
    if (!huf_only_frame(frame, j[1], rs, ho)) {
      if (lane == 0 && stream == 0) status[pg] = 1;
      continue;
    }
    if (stream >= ho.nStreams) continue;
    const uint8_t* p = frame + ho.payload;
    const int64_t descLen = ho.cs < kHufDescMax ? ho.cs : kHufDescMax;
    if (lane < descLen) c.desc[lane] = p[lane];
    __syncthreads();
    // a description is at most kHufDescMax bytes, so the copy's length
    // stands in for cs
    if (lane == 0) c.used = read_huf_tree(c.desc, descLen, c.huf, c.ws);
    __syncthreads();
    const int64_t used = c.used;
    HufParStream s;
    bool ok = used >= 0 &&
              huf_par_stream(p + used, ho.cs - used, rs, ho.nStreams, stream, s);
    if (!ok) {
      if (lane == 0) status[pg] = 1;
      __syncthreads();  // c is reused by the next item
      continue;
    }
    const int32_t S = huf_lane_span(s.T, kHufLanes);
    const int32_t bEnd = huf_lane_top(s.T, S, lane + 1);
    int32_t start = huf_lane_top(s.T, S, lane);
    HufLaneExit r = huf_lane_scan(c.huf, s.src, start, bEnd);
    // fix-up: lanes 0..k are right after round k, so kHufLanes rounds
    // always suffice and the last one finds nothing to change
    bool settled = false;
    for (int round = 0; round <= kHufLanes; round++) {
      c.exitb[lane] = r.b;
      __syncthreads();
      const int32_t prev = lane > 0 ? c.exitb[lane - 1] : start;
      const bool changed = prev != start;
      if (!__syncthreads_or(changed)) {  // also fences exitb for the next round
        settled = true;
        break;
      }
      if (changed) {
        start = prev;
        r = huf_lane_scan(c.huf, s.src, start, bEnd);
      }
    }
    // offsets: exclusive prefix sum of the counts over the workgroup
    const int wave = lane >> 6, wlane = lane & 63;
    const int32_t incl = wave_scan(r.count, wlane);
    if (wlane == 63) c.wsum[wave] = incl;
    __syncthreads();
    int32_t before = 0, total = 0;
    for (int w = 0; w < kHufWaves; w++) {
      if (w < wave) before += c.wsum[w];
      total += c.wsum[w];
    }
    ok = settled && total == s.outLen && c.exitb[kHufLanes - 1] == 0;
    if (ok)
      huf_lane_write(c.huf, s.src, start, r.count,
                     dst + j[2] + s.outStart + before + (incl - r.count));
    else if (lane == 0)
      status[pg] = 1;
    __syncthreads();  // c is reused by the next item
  }
}

}  // namespace lsz_gpu

namespace lakesoul {

void launch_zstd_huf_decompress(const uint8_t* src, const int64_t* jobs,
                                int64_t njobs, uint8_t* dst, int32_t* status,
                                hipStream_t stream) {
  if (njobs == 0) return;
  (void)hipMemsetAsync(status, 0, (size_t)njobs * sizeof(int32_t), stream);
  // a workgroup per (page, stream); beyond what fills every CU several
  // times over they share the items grid-stride
  int64_t items = 4 * njobs;
  int64_t nblocks = items < 8192 ? items : 8192;
  hipLaunchKernelGGL(lsz_gpu::zstd_huf_pages_kernel, dim3((uint32_t)nblocks),
                     dim3(lsz_gpu::kHufLanes), 0, stream, src, jobs, njobs, dst,
                     status);
}

}  // namespace lakesoul
