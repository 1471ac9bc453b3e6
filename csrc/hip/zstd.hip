// GPU zstd page decompressor (gfx950): one wave64 workgroup per parquet
// page, grid-stride over pages. Shared with the host reference
// implementation (csrc/cpp/zstd_dec.h, differential-tested against
// libzstd): the bit readers, the FSE / huffman table builders and every
// format parse function (frame, block and literals headers, huffman tree
// description, 4-stream layout, sequence count, sequence tables, one
// sequence). Every lane calls the parse functions on the same bytes, so
// their results and every early return are lane-uniform; the ones that
// build a table run on lane 0 only. This file holds what is per-side —
// the byte movement and its fencing, i.e. the CDNA4 execution strategy:
//
// - every lane runs the *sequential* control flow redundantly in
//   lockstep (same bytes, same results — no broadcasts, no divergence);
// - byte copies (raw blocks, literals, matches) fan out across all 64
//   lanes; overlapping matches use period replication
//   (dst[out+j] = dst[out-offset + j%offset], reads strictly below out);
// - FSE/huffman decode tables live in LDS (~10.5 KB — wave-coherent, no
//   fences); the 128 KB literals buffer is per-workgroup global scratch;
// - 4-stream huffman literals decode on 4 lanes concurrently;
// - cross-lane visibility of cooperative copies uses the proven snappy
//   kernel pattern: volatile (GLC) reads of wave-written regions +
//   s_waitcnt(0) after each cooperative segment.
//
// Throughput comes from pages in flight (thousands per scan unit), not
// from single-page speed — decompression scales with the GPU instead of
// the cgroup-capped host CPU quota.

#include <hip/hip_runtime.h>

#include "../cpp/zstd_dec.h"
#include "kernels.h"
#include "wave_copy.h"

namespace lsz_gpu {

using namespace lszstd;
using namespace lswave;  // waitcnt0, wcopy_wide, wcopy_src

#define LANES 64
static const int kLitBufCap = 1 << 17;  // 128 KB literals per block

// order LDS ops only (lgkmcnt(0); vmcnt=63, expcnt=7 untouched): the
// window read/write shuffle must not drain in-flight global stores —
// a full __syncthreads here costs ~1000 cycles per sequence (measured,
// profiles/r01_gpu_zstd.md)
__device__ inline void lds_sync() { __builtin_amdgcn_s_waitcnt(0xC07F); }

// cooperative copy from the literals scratch (written by this wave
// earlier — volatile read to bypass stale L1)
__device__ inline void wcopy_from_lit(uint8_t* dst, const uint8_t* lit,
                                      uint32_t len, int lane) {
  wcopy_wide<true>(dst, lit, len, lane);
  waitcnt0();
}

__device__ inline void wfill(uint8_t* dst, uint8_t v, int64_t len, int lane) {
  uint64_t w = 0x0101010101010101ull * v;
  int64_t n8 = len >> 3;
  for (int64_t j = lane; j < n8; j += LANES) *(uint64_t*)(dst + 8 * j) = w;
  for (int64_t j = (n8 << 3) + lane; j < len; j += LANES) dst[j] = v;
  waitcnt0();
}

struct LdsCtx {
  SeqTables seq;
  HufTable huf;
  bool haveHuf;
  int64_t scratch_i64;     // lane0 -> wave value handoff
  // lane0 table-build workspace (LDS, not per-lane scratch memory —
  // dynamically-indexed locals would otherwise force a multi-KB private
  // segment that craters wave residency)
  BuildWs ws;
  // rolling window of the last 32 output bytes (win[31] most recent).
  // Matches with offset <= 32 read ONLY this window: no global reads,
  // no fences — the serial cost per sequence collapses to LDS ops.
  uint8_t win[32];
};

// window <- last 32 bytes of (window ++ run): BYTE_AT is an expression in
// k (int64_t) that yields byte k of the n-byte appended run. Every lane
// reads its new byte before any lane writes; SYNC orders the two (and
// follows the write): __syncthreads, or lds_sync inside the sequence loop.
// A macro, not a function taking a callable: through a function the
// compiler laid the in-loop sites out with two more LDS reads and four
// more LDS waits per sequence (3.6 % slower on sorted int64 pages).
#define WIN_SLIDE(c, n, lane, SYNC, BYTE_AT)                          \
  do {                                                                \
    uint8_t nb_ = 0;                                                  \
    if ((lane) < 32) {                                                \
      int64_t w_ = (int64_t)(lane) + (n); /* index into window ++ run */ \
      int64_t k = w_ - 32;                                            \
      nb_ = (w_ < 32) ? (c).win[w_] : (BYTE_AT);                      \
    }                                                                 \
    SYNC();                                                           \
    if ((lane) < 32) (c).win[lane] = nb_;                             \
    SYNC();                                                           \
  } while (0)

// slide `src[0..n)` into the 32-byte window (volatile read: src may be
// wave-written global memory that has been fenced)
__device__ inline void win_append_from(LdsCtx& c, const uint8_t* src,
                                       int64_t n, int lane) {
  if (n <= 0) return;
  WIN_SLIDE(c, n, lane, __syncthreads, ((volatile const uint8_t*)src)[k]);
}

__device__ inline void win_fill(LdsCtx& c, uint8_t v, int lane) {
  if (lane < 32) c.win[lane] = v;
  __syncthreads();
}

// decode the literals section. All lanes in lockstep; table builds by
// lane 0 into LDS; stream decode on up to 4 lanes. Returns bytes
// consumed from src or -1; litLen receives the regenerated length.
__device__ inline int64_t dev_literals(LdsCtx& c, uint8_t* lit,
                                       const uint8_t* src, int64_t n,
                                       int64_t& litLen, int lane) {
  LitHdr h;
  if (!parse_literals_header(src, n, h)) return -1;
  if (h.rs > kLitBufCap) return -1;
  litLen = h.rs;
  const uint8_t* p = src + h.hdr;
  if (h.type == kLitRaw) {
    wcopy_src(lit, p, h.rs, lane);
    return h.hdr + h.cs;
  }
  if (h.type == kLitRle) {
    wfill(lit, p[0], h.rs, lane);
    return h.hdr + h.cs;
  }
  int64_t rem = h.cs;
  if (h.type == kLitCompressed) {
    // weights parse + table build on lane 0 only (keeps the 256-byte
    // weights array and FSE decode state out of per-lane scratch)
    if (lane == 0) {
      int64_t used = read_huf_tree(p, rem, c.huf, c.ws);
      if (used >= 0) c.haveHuf = true;
      c.scratch_i64 = used;
    }
    __syncthreads();
    if (c.scratch_i64 < 0) return -1;
    p += c.scratch_i64;
    rem -= c.scratch_i64;
    __syncthreads();
  } else if (!c.haveHuf) {
    return -1;
  }

  bool ok = true;
  if (h.nStreams == 1) {
    if (lane == 0) ok = huf_stream(c.huf, p, rem, lit, h.rs);
  } else {
    HufStream s;
    if (!huf4_stream(p, rem, h.rs, lane & 3, s)) return -1;
    if (lane < 4)  // one shared decode instance: lanes 0-3 each take a stream
      ok = huf_stream(c.huf, p + s.start, s.len, lit + s.outStart, s.outLen);
  }
  waitcnt0();
  __syncthreads();
  if (__ballot(!ok)) return -1;
  return h.hdr + h.cs;
}

// one sequence table: lane 0 builds it in LDS and hands the bytes
// consumed to the wave. Repeat mode builds nothing, so every lane
// evaluates it and there is no handoff and no barrier.
__device__ inline int64_t dev_read_seq_table(LdsCtx& c, int kind, int mode,
                                             const uint8_t* src, int64_t n,
                                             int lane) {
  if (mode == kModeRepeat) return read_seq_table(c.seq, kind, mode, src, n, c.ws);
  if (lane == 0) c.scratch_i64 = read_seq_table(c.seq, kind, mode, src, n, c.ws);
  __syncthreads();
  return c.scratch_i64;
}

// one compressed block; every lane in lockstep
__device__ inline int64_t dev_block(LdsCtx& c, uint8_t* lit, uint32_t* rep,
                                    const uint8_t* src, int64_t n,
                                    uint8_t* dstBase, int64_t pos,
                                    int64_t dstCap, int lane) {
  int64_t litLen;
  int64_t used = dev_literals(c, lit, src, n, litLen, lane);
  if (used < 0) return -1;
  const uint8_t* p = src + used;
  int64_t rem = n - used;

  int64_t nSeq;
  used = read_seq_count(p, rem, nSeq);
  if (used < 0) return -1;
  p += used; rem -= used;

  if (nSeq == 0) {
    if (pos + litLen > dstCap) return -1;
    wcopy_from_lit(dstBase + pos, lit, (uint32_t)litLen, lane);
    win_append_from(c, lit, litLen, lane);
    return litLen;
  }

  if (rem < 1) return -1;
  uint8_t modes = p[0];
  p += 1; rem -= 1;
  for (int kind = kSeqLL; kind <= kSeqML; kind++) {
    used = dev_read_seq_table(c, kind, seq_mode(modes, kind), p, rem, lane);
    if (used < 0) return -1;
    p += used; rem -= used;
  }

  BitBwd br;
  if (!br.init(p, rem)) return -1;
  SeqStates ss;
  ss.init(c.seq, br);

  // W = everything below this output position is store-fence'd (visible
  // to plain/GLC reads); advance lazily, fencing only when a large-offset
  // match must read not-yet-fenced bytes
  int64_t W = pos;
  int64_t litPos = 0;
  int64_t out = pos;
  for (int64_t s = 0; s < nSeq; s++) {
    Seq q = next_sequence(c.seq, ss, br, rep);
    uint32_t litLenSeq = q.litLen, matchLen = q.matchLen, offset = q.offset;

    // ---- literals: litBuf reads are hazard-free (fenced after the
    // literals phase); dst writes are fire-and-forget ----
    if (litPos + litLenSeq > litLen || out + litLenSeq > dstCap) return -1;
    if (litLenSeq) {
      wcopy_wide<true>(dstBase + out, lit + litPos, litLenSeq, lane);
      WIN_SLIDE(c, litLenSeq, lane, lds_sync,
                ((volatile const uint8_t*)lit)[litPos + k]);
      litPos += litLenSeq;
      out += litLenSeq;
    }

    // ---- match ----
    if ((int64_t)offset > out || out + matchLen > dstCap) return -1;
    if (offset <= 32) {
      // source is entirely inside the register window: no global reads
      for (uint32_t j = lane; j < matchLen; j += LANES)
        dstBase[out + j] = c.win[(32 - offset) + (j % offset)];
      WIN_SLIDE(c, matchLen, lane, lds_sync,
                c.win[(32 - offset) + (uint32_t)(k % offset)]);
    } else {
      // large offset: source bytes live below `out`; fence once if they
      // reach into the unfenced region
      uint32_t span = offset < matchLen ? offset : matchLen;
      if (out - (int64_t)offset + (int64_t)span > W) {
        waitcnt0();
        W = out;
      }
      for (uint32_t j = lane; j < matchLen; j += LANES)
        dstBase[out + j] =
            ((volatile const uint8_t*)dstBase)[out - offset + (j % offset)];
      WIN_SLIDE(c, matchLen, lane, lds_sync,
                ((volatile const uint8_t*)
                     dstBase)[out - offset + (uint32_t)(k % offset)]);
    }
    out += matchLen;

    if (s + 1 < nSeq) {  // last sequence: no state update
      ss.update(c.seq, br);
      if (br.overflow) return -1;
    }
  }
  int64_t tail = litLen - litPos;
  if (tail < 0 || out + tail > dstCap) return -1;
  wcopy_from_lit(dstBase + out, lit + litPos, (uint32_t)tail, lane);
  win_append_from(c, lit + litPos, tail, lane);
  out += tail;
  return out - pos;
}

__device__ inline int64_t dev_frame(LdsCtx& c, uint8_t* lit, const uint8_t* src,
                                    int64_t n, uint8_t* dst, int64_t dstCap,
                                    int lane) {
  int64_t pos = 0, ip = 0;
  uint32_t rep[3];
  while (ip + 4 <= n) {
    bool skippable, checksum;
    ip = parse_frame_header(src, n, ip, skippable, checksum);
    if (ip < 0) return -1;
    if (skippable) continue;

    if (lane == 0) {
      c.seq.have[0] = c.seq.have[1] = c.seq.have[2] = false;
      c.haveHuf = false;
    }
    if (lane < 32) c.win[lane] = 0;
    __syncthreads();
    rep[0] = 1; rep[1] = 4; rep[2] = 8;

    BlockHdr b;
    do {
      if (!parse_block_header(src + ip, n - ip, b)) return -1;
      ip += 3;
      if (b.type == kBlockCompressed) {
        int64_t outb = dev_block(c, lit, rep, src + ip, b.size, dst, pos,
                                 dstCap, lane);
        if (outb < 0) return -1;
        pos += outb;
      } else {
        if (pos + b.size > dstCap) return -1;
        if (b.type == kBlockRaw) {
          wcopy_src(dst + pos, src + ip, b.size, lane);
          win_append_from(c, src + ip, b.size, lane);
        } else {
          uint8_t v = src[ip];
          wfill(dst + pos, v, b.size, lane);
          if (b.size >= 32)
            win_fill(c, v, lane);
          else
            WIN_SLIDE(c, b.size, lane, __syncthreads, ((void)k, v));
        }
        pos += b.size;
      }
      ip += b.srcBytes;
    } while (!b.last);
    if (checksum) ip += 4;
  }
  return pos;
}

__global__ void __launch_bounds__(LANES, 4) zstd_pages_kernel(
    const uint8_t* __restrict__ src, const int64_t* __restrict__ jobs,
    int64_t njobs, uint8_t* __restrict__ dst, uint8_t* __restrict__ scratch,
    int32_t* __restrict__ status) {
  __shared__ LdsCtx c;
  int lane = threadIdx.x;
  uint8_t* lit = scratch + (int64_t)blockIdx.x * kLitBufCap;
  for (int64_t p = blockIdx.x; p < njobs; p += gridDim.x) {
    const int64_t* j = jobs + 4 * p;
    int64_t r = dev_frame(c, lit, src + j[0], j[1], dst + j[2], j[3], lane);
    if (lane == 0) status[p] = (r == j[3]) ? 0 : 1;
    __syncthreads();
  }
}

}  // namespace lsz_gpu

namespace lakesoul {

void launch_zstd_decompress(const uint8_t* src, const int64_t* jobs,
                            int64_t njobs, uint8_t* dst, uint8_t* scratch,
                            int64_t nblocks, int32_t* status,
                            hipStream_t stream) {
  if (njobs == 0) return;
  dim3 grid((uint32_t)nblocks), block(LANES);
  hipLaunchKernelGGL(lsz_gpu::zstd_pages_kernel, grid, block, 0, stream, src,
                     jobs, njobs, dst, scratch, status);
}

int64_t lsz_gpu_litbuf_bytes() { return lsz_gpu::kLitBufCap; }

}  // namespace lakesoul
