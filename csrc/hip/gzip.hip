// DEFLATE decompression on the GPU (gfx950), parquet codec 2 (GZIP): one
// wave64 workgroup per page, grid-stride over pages.
//
// A page is one or more gzip members, or one zlib stream; each holds a
// DEFLATE stream of stored, fixed-Huffman and dynamic-Huffman blocks.
// - Every lane runs the parse on the same bytes through the functions of
//   csrc/cpp/inflate.h, shared with the host decoder: the bit reader, the
//   framing and block headers, the table builder and parse_symbol. The
//   control flow and every early exit are wave-uniform: no broadcasts.
// - Both decode tables (852 + 592 entries of 4 bytes) and the builder's
//   workspace live in LDS; a table read is a same-address broadcast. The
//   lanes split the replicated entries of the table fill
//   (lsinfl::build_table(lane, 64); the host runs lane 0 of 1, and
//   csrc/cpp/tests/inflate_san.cc checks that both give one table).
// - A DEFLATE literal is one symbol and one byte: literal k of a run is
//   held in lane k % 64, and up to 64 of them leave as one coalesced store
//   when the batch fills, before a match and at the end of a block.
// - Matches copy inside the output with all 64 lanes (wave_copy.h): 8 bytes
//   per lane when the source lies wholly below the match, by period
//   replication when it overlaps. They read bytes other lanes stored:
//   volatile (GLC) loads, and the wave drains its stores (s_waitcnt(0))
//   only before a match whose source reaches above the last drained
//   position `fenced`, as lz4.hip does. A literal flush and a stored block
//   (copied from the source, 8 bytes per lane) leave undrained stores.
//
// Checks: every check of the host decoder's stream walk (inflate_stream),
// the framing, ISIZE of each gzip member and the exact output length. The
// kernel does NOT compute CRC32 or Adler-32: a page whose bytes were
// damaged in a way that still parses is caught by the host route only. A
// bad page gets a non-zero status and nothing outside its own output range
// is written.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
// 119 VGPRs, 106 SGPRs, no scratch, 6756 bytes of LDS per workgroup,
// 4 waves per SIMD. Measured: profiles/r08_gpu_gzip.md; the scan route is
// off by default (LAKESOUL_GPU_GZIP=1 turns it on).

#include <hip/hip_runtime.h>

// the lanes' meeting point in lsinfl::build_table (device code only: the
// host half of this translation unit builds no table)
#if defined(__HIP_DEVICE_COMPILE__)
#define LSINFL_SYNC() __syncthreads()
#endif
#include "../cpp/inflate.h"
#include "kernels.h"
#include "wave_copy.h"

namespace lakesoul {

using namespace lswave;

// jobs: int64 [n][4] = {src_off, src_len, dst_off, dst_len}
// status[i]: 0 ok, nonzero error
__global__ void __launch_bounds__(kLanes) inflate_pages_kernel(
    const uint8_t* __restrict__ src_buf, const int64_t* __restrict__ jobs,
    int64_t njobs, uint8_t* __restrict__ dst_buf, int32_t* __restrict__ status) {
  __shared__ lsinfl::Tables T;
  __shared__ lsinfl::Work W;
  const int lane = threadIdx.x;
  for (int64_t p = blockIdx.x; p < njobs; p += gridDim.x) {
    const int64_t* job = jobs + 4 * p;
    const uint8_t* src = src_buf + job[0];
    const int64_t n = job[1];
    uint8_t* dst = dst_buf + job[2];
    const int64_t cap = job[3];

    int err = 0;
    // parquet page sizes are int32; the match copy indexes in 32 bits
    if (n < 2 || cap < 0 || n > 0x7fffffff || cap > 0x7fffffff) err = 1;
    const bool gz = !err && lsinfl::is_gzip(src, n);
    int64_t pos = 0;   // in src
    int64_t done = 0;  // output of the members before this one
    while (!err) {     // one gzip member, or the zlib stream, per round
      if (!(gz ? lsinfl::gzip_header(src, n, pos) : lsinfl::zlib_header(src, n, pos))) {
        err = 2;
        break;
      }
      uint8_t* out = dst + done;  // distances count back from here
      const int64_t room = cap - done;
      lsinfl::Bits b;
      lsinfl::bits_init(b, src, n, pos);
      int64_t d = 0;
      int64_t fenced = 0;  // stores below out + fenced have been drained
      bool have_fixed = false;
      uint32_t mylit = 0;  // literal `lane` of the open batch
      int nlit = 0;        // literals in the open batch, not yet in d
      bool last = false;
      while (!err && !last) {
        lsinfl::Block blk;
        if (!lsinfl::parse_block_header(b, blk)) { err = 3; break; }
        last = blk.last;
        if (blk.kind == lsinfl::BLK_STORED) {
          if ((int64_t)blk.stored_len > room - d) { err = 4; break; }
          wcopy_wide<false>(out + d, src + blk.stored_pos, blk.stored_len, lane);
          d += blk.stored_len;
          continue;
        }
        if (blk.kind == lsinfl::BLK_FIXED) {
          if (!have_fixed && !lsinfl::build_fixed(T, W, lane, kLanes)) { err = 5; break; }
          have_fixed = true;
        } else {
          have_fixed = false;
          if (!lsinfl::build_dynamic(b, T, W, lane, kLanes)) { err = 6; break; }
        }
        for (;;) {
          lsinfl::Sym s;
          const int k = lsinfl::parse_symbol(b, T, s);
          if (k == lsinfl::SYM_LIT) {
            if (d + nlit >= room) { err = 7; break; }
            if (lane == nlit) mylit = s.lit;
            if (++nlit < kLanes) continue;
          } else if (k == lsinfl::SYM_BAD) {
            err = 8;
            break;
          }
          // a full batch, a match or the end of the block: the literals go
          if (lane < nlit) out[d + lane] = (uint8_t)mylit;
          d += nlit;
          nlit = 0;
          if (k == lsinfl::SYM_END) break;
          if (k != lsinfl::SYM_MATCH) continue;
          if ((int64_t)s.dist > d) { err = 9; break; }
          if ((int64_t)s.len > room - d) { err = 10; break; }
          const uint32_t off = s.dist, ml = s.len;
          // source bytes are [d - off, d - off + min(off, ml))
          if (d - off + (off < ml ? off : ml) > fenced) {
            waitcnt0();
            fenced = d;
          }
          if (off >= ml) {
            wcopy_wide<true>(out + d, out + d - off, ml, lane);
          } else {
            wcopy_match(out, d, off, ml, lane);  // drains its stores
            fenced = d + ml;
          }
          d += ml;
        }
      }
      if (err) break;
      pos = lsinfl::byte_align(b);
      if (b.bad) { err = 11; break; }
      if (!gz) {  // Adler-32 follows and ends the page; it is not computed
        if (n - pos != 4) err = 12;
        done += d;
        break;
      }
      if (n - pos < 8) { err = 13; break; }
      if (lsinfl::le32(src + pos + 4) != (uint32_t)d) { err = 14; break; }  // ISIZE
      pos += 8;  // CRC32 is not computed
      done += d;
      if (pos >= n) break;
    }
    if (!err && done != cap) err = 15;
    if (lane == 0) status[p] = err;
  }
}

void launch_gzip_decompress(const uint8_t* src, const int64_t* jobs,
                            int64_t njobs, uint8_t* dst, int32_t* status,
                            hipStream_t stream) {
  if (njobs <= 0) return;
  int64_t blocks = njobs < 2048 ? njobs : 2048;
  hipLaunchKernelGGL(inflate_pages_kernel, dim3((uint32_t)blocks), dim3(kLanes), 0,
                     stream, src, jobs, njobs, dst, status);
}

}  // namespace lakesoul
