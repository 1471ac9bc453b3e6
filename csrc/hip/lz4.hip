// LZ4 block decompression on the GPU (gfx950), parquet codec 7 (LZ4_RAW):
// one wave64 workgroup per page, grid-stride over pages.
//
// A block is a chain of sequences (token, literals, match) and has no
// entropy stage, so a page costs a token walk plus byte copies:
// - every lane runs the token walk on the same bytes through
//   lslz4::lz4_parse_seq (csrc/cpp/lz4_dec.h, shared with the host decoder),
//   so the control flow and every early exit are wave-uniform: no
//   broadcasts, no divergence, no LDS;
// - all 64 lanes move the bytes: literals from the read-only source,
//   8 bytes per lane with a byte tail; matches from the output, 8 bytes per
//   lane when the source lies wholly below the match, by period replication
//   (dst[d+j] = dst[d-off + j%off], reads strictly below d) when the match
//   overlaps itself;
// - a match may read bytes that other lanes stored in this or an earlier
//   sequence: those reads are volatile (GLC), and the wave drains its
//   stores (s_waitcnt(0)) before a match whose source reaches above the
//   last drained position `fenced`. Literal stores are fire-and-forget.
//
// The bounds checks are the host decoder's (lz4_block_decode): a damaged
// page gets a non-zero status and nothing outside its own output range is
// written.
//
// Throughput comes from pages in flight, not single-page speed. Measured
// (profiles/r04_gpu_lz4.md): literal-only pages copy at 1.5-1.9 TB/s; pages
// of short matches behind the write position (sorted ids, small integers)
// pay one store drain per sequence, about 1 us, and reach 11-19 GB/s with
// 4096 pages in flight. A scan unit holds a few hundred pages, so the scan
// route is off by default (LAKESOUL_GPU_LZ4=1 turns it on). 26 VGPRs, no
// scratch, no LDS.

#include <hip/hip_runtime.h>

#include "../cpp/lz4_dec.h"
#include "kernels.h"
#include "wave_copy.h"

namespace lakesoul {

using namespace lswave;

// jobs: int64 [n][4] = {src_off, src_len, dst_off, dst_len}
// status[i]: 0 ok, nonzero error
__global__ void __launch_bounds__(kLanes) lz4_pages_kernel(
    const uint8_t* __restrict__ src_buf, const int64_t* __restrict__ jobs,
    int64_t njobs, uint8_t* __restrict__ dst_buf, int32_t* __restrict__ status) {
  const int lane = threadIdx.x;
  for (int64_t p = blockIdx.x; p < njobs; p += gridDim.x) {
    const int64_t* job = jobs + 4 * p;
    const uint8_t* src = src_buf + job[0];
    const int64_t n = job[1];
    uint8_t* dst = dst_buf + job[2];
    const int64_t cap = job[3];

    int err = 0;
    // parquet page sizes are int32; the match copy indexes in 32 bits
    if (n < 0 || cap < 0 || n > 0x7fffffff || cap > 0x7fffffff) err = 1;
    int64_t pos = 0, d = 0;
    int64_t fenced = 0;  // stores below dst + fenced have been drained
    while (!err) {
      lslz4::Seq q;
      if (!lslz4::lz4_parse_seq(src, n, pos, q)) { err = 2; break; }
      if (q.lit_len > (uint64_t)(cap - d)) { err = 3; break; }
      wcopy_wide<false>(dst + d, src + q.lit_pos, (int64_t)q.lit_len, lane);
      d += (int64_t)q.lit_len;
      if (q.last) {
        if (d != cap) err = 4;
        break;
      }
      if (q.offset == 0 || (int64_t)q.offset > d) { err = 5; break; }
      if (q.match_len > (uint64_t)(cap - d)) { err = 6; break; }
      const uint32_t off = q.offset, ml = (uint32_t)q.match_len;
      // source bytes are [d - off, d - off + min(off, ml))
      if (d - off + (off < ml ? off : ml) > fenced) {
        waitcnt0();
        fenced = d;
      }
      if (off >= ml) {
        wcopy_wide<true>(dst + d, dst + d - off, ml, lane);
      } else {
        wcopy_match(dst, d, off, ml, lane);  // drains its stores
        fenced = d + ml;
      }
      d += ml;
      pos = q.next;
    }
    if (lane == 0) status[p] = err;
  }
}

void launch_lz4_decompress(const uint8_t* src, const int64_t* jobs,
                           int64_t njobs, uint8_t* dst, int32_t* status,
                           hipStream_t stream) {
  if (njobs <= 0) return;
  int64_t blocks = njobs < 2048 ? njobs : 2048;
  hipLaunchKernelGGL(lz4_pages_kernel, dim3((uint32_t)blocks), dim3(kLanes), 0,
                     stream, src, jobs, njobs, dst, status);
}

}  // namespace lakesoul
