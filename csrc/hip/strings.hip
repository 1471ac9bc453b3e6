// String bytes of a scan unit moved on the GPU (gfx950): a byte-parallel
// segment copy. A string column's output is a run of segments (values) laid
// end to end; `off` holds their nseg + 1 destination offsets. Parallelism
// follows the OUTPUT BYTES, not the rows: a column of 3-byte values keeps
// every lane busy, and a 70 KB value is spread over many workgroups.
//
// - A 256-thread workgroup owns a tile of kTile output bytes and
//   grid-strides over the tiles (at most 2048 workgroups). Tiles are cut on
//   8-byte boundaries of the destination ADDRESS, so every word a thread
//   produces is an aligned 8-byte store; only the first and the last word of
//   the buffer can be partial and are stored bytewise.
// - The owner of a byte is found by an upper-bound search in the offsets
//   (lsseg::owner, csrc/cpp/str_seg.h, shared with the host twin), so runs of
//   empty values are skipped, not visited. Thread 0 finds the tile's first
//   and last segment; when that slice of the offsets fits kStage entries it
//   is staged in LDS and the per-word searches run there, otherwise they run
//   on the same slice in global memory.
// - Two sources share the body: the PLAIN stream with its length prefixes
//   stripped (src = raw + b + 4 * (i + 1)) and a dictionary
//   (src = dict_bytes + dict_off[entry[i]] + (b - off[i])).
// - A word that lies inside one segment is assembled from aligned dword
//   loads (three when the source is not dword-aligned); a word that crosses
//   segments, or sits at the edge of the source buffer, from byte loads. No
//   unaligned pointer is cast.
// - Every source index is checked against the source buffer: a byte whose
//   source lies outside reads as 0, whatever the tables hold.

#include <hip/hip_runtime.h>

#include "../cpp/str_seg.h"
#include "kernels.h"

namespace lakesoul {

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 4096;    // output bytes per workgroup trip
constexpr int kStage = 2048;   // offsets staged in LDS (16 KB)
constexpr int kMaxBlocks = 2048;

struct SegSrc {
  const uint8_t* src;       // raw PLAIN stream, or stripped dictionary bytes
  int64_t src_len;
  const int64_t* dict_off;  // dictionary: entry offsets (nent + 1)
  int64_t nent;
  const int32_t* entry;     // dictionary: entry of each segment, -1 = none
};

// source index minus output index for the bytes of segment `seg`
// (o = offsets of the tile's slice, whose first segment is `first`)
template <bool DICT>
__device__ __forceinline__ bool seg_delta(const SegSrc& s, const int64_t* o,
                                          int64_t first, int64_t seg,
                                          int64_t& delta) {
  if (!DICT) {
    delta = lsseg::strip_delta(first + seg);
    return true;
  }
  return lsseg::dict_delta(s.dict_off, s.nent, s.entry[first + seg], o[seg], delta);
}

__device__ __forceinline__ uint64_t load_byte(const SegSrc& s, int64_t si) {
  return si >= 0 && si < s.src_len ? (uint64_t)s.src[si] : 0;
}

// 8 source bytes from index si, little-endian
__device__ __forceinline__ uint64_t load_word(const SegSrc& s, int64_t si) {
  if (si >= 0 && si + 8 <= s.src_len) {
    uintptr_t p = (uintptr_t)(s.src + si);
    uintptr_t a = p & ~(uintptr_t)3;
    uint32_t sh = (uint32_t)(p & 3) * 8;
    if (a >= (uintptr_t)s.src &&
        a + (sh ? 12 : 8) <= (uintptr_t)s.src + (uintptr_t)s.src_len) {
      const uint32_t* q = (const uint32_t*)a;
      uint32_t d0 = q[0], d1 = q[1];
      if (!sh) return (uint64_t)d0 | ((uint64_t)d1 << 32);
      uint32_t d2 = q[2];
      uint32_t lo = (d0 >> sh) | (d1 << (32 - sh));
      uint32_t hi = (d1 >> sh) | (d2 << (32 - sh));
      return (uint64_t)lo | ((uint64_t)hi << 32);
    }
  }
  uint64_t w = 0;
  for (int k = 0; k < 8; k++) w |= load_byte(s, si + k) << (8 * k);
  return w;
}

// output bytes [bs, be) (at most 8; a full word when be - bs == 8) from the
// tile's slice of the offsets: o[0 .. nrel], first segment `first`
template <bool DICT>
__device__ __forceinline__ void copy_word(const SegSrc& s, const int64_t* o,
                                          int64_t nrel, int64_t first,
                                          uint8_t* dst, int64_t bs, int64_t be) {
  int64_t sg = lsseg::owner(o, 0, nrel, bs);
  int64_t seg_end = o[sg + 1];
  int64_t delta = 0;
  bool have = seg_delta<DICT>(s, o, first, sg, delta);
  const bool full = be - bs == 8;
  uint64_t w = 0;
  if (full && seg_end >= be) {
    if (have) w = load_word(s, bs + delta);
  } else {
    for (int64_t b = bs; b < be; b++) {
      if (b >= seg_end && sg + 1 < nrel) {
        sg++;
        if (o[sg + 1] <= b) sg = lsseg::owner(o, sg, nrel, b);
        seg_end = o[sg + 1];
        have = seg_delta<DICT>(s, o, first, sg, delta);
      }
      if (have) w |= load_byte(s, b + delta) << (8 * (b - bs));
    }
  }
  if (full) {
    *(uint64_t*)(dst + bs) = w;  // aligned: tiles are cut on the address
  } else {
    for (int64_t b = bs; b < be; b++) dst[b] = (uint8_t)(w >> (8 * (b - bs)));
  }
}

template <bool DICT>
__global__ void __launch_bounds__(kThreads) seg_copy_kernel(
    SegSrc s, const int64_t* __restrict__ off, int64_t nseg,
    uint8_t* __restrict__ dst, int64_t total) {
  __shared__ int64_t stage[kStage];
  __shared__ int64_t s_lo, s_hi;
  // v = b + mis: position counted from the 8-byte boundary at or below dst
  const int64_t mis = (int64_t)((uintptr_t)dst & 7);
  const int64_t vtotal = mis + total;
  const int64_t ntiles = (vtotal + kTile - 1) / kTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t v0 = t * kTile;
    const int64_t v1 = v0 + kTile < vtotal ? v0 + kTile : vtotal;
    const int64_t b0 = v0 > mis ? v0 - mis : 0, b1 = v1 - mis;
    if (threadIdx.x == 0) {
      int64_t lo = lsseg::owner(off, 0, nseg, b0);
      s_lo = lo;
      s_hi = lsseg::owner(off, lo, nseg, b1 - 1);
    }
    __syncthreads();
    const int64_t first = s_lo, nrel = s_hi - s_lo + 1;
    const bool staged = nrel + 1 <= kStage;
    if (staged)
      for (int64_t i = threadIdx.x; i <= nrel; i += kThreads)
        stage[i] = off[first + i];
    __syncthreads();
    for (int64_t v = v0 + 8 * (int64_t)threadIdx.x; v < v1; v += 8 * kThreads) {
      int64_t bs = v > mis ? v - mis : 0;
      int64_t be = v + 8 < vtotal ? v + 8 - mis : total;
      if (be <= bs) continue;  // the word below a misaligned dst
      if (staged)
        copy_word<DICT>(s, stage, nrel, first, dst, bs, be);
      else
        copy_word<DICT>(s, off + first, nrel, first, dst, bs, be);
    }
    __syncthreads();  // stage and s_lo / s_hi are rewritten by the next trip
  }
}

// one thread per row of a dictionary string column: its value's length and
// entry (lsseg::dict_row_len, shared with the host twin)
__global__ void __launch_bounds__(kThreads) dict_str_lens_kernel(
    const int32_t* __restrict__ idx, int64_t n_idx,
    const int64_t* __restrict__ dict_off, int64_t nent,
    const uint8_t* __restrict__ validity, const int64_t* __restrict__ pos,
    int64_t nrows, int64_t* __restrict__ lens, int32_t* __restrict__ entry,
    int32_t* __restrict__ status) {
  for (int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x; r < nrows;
       r += (int64_t)gridDim.x * kThreads) {
    bool valid = !validity || validity[r];
    int32_t e, st;
    lens[r] = lsseg::dict_row_len(idx, n_idx, dict_off, nent, valid,
                                  validity ? (valid ? pos[r] : 0) : r, e, st);
    entry[r] = e;
    if (st) atomicOr(status, st);
  }
}

template <bool DICT>
void launch_seg_copy(const SegSrc& s, const int64_t* off, int64_t nseg,
                     uint8_t* dst, int64_t total, hipStream_t stream) {
  if (total <= 0 || nseg <= 0) return;
  int64_t ntiles = (total + 7 + kTile - 1) / kTile;
  int64_t blocks = ntiles < kMaxBlocks ? ntiles : kMaxBlocks;
  hipLaunchKernelGGL(seg_copy_kernel<DICT>, dim3((uint32_t)blocks),
                     dim3(kThreads), 0, stream, s, off, nseg, dst, total);
}

}  // namespace

void launch_strip_prefixes(const uint8_t* raw, int64_t raw_len,
                           const int64_t* dense_off, int64_t n, uint8_t* dst,
                           int64_t total, hipStream_t stream) {
  SegSrc s{raw, raw_len, nullptr, 0, nullptr};
  launch_seg_copy<false>(s, dense_off, n, dst, total, stream);
}

void launch_dict_str_lens(const int32_t* idx, int64_t n_idx,
                          const int64_t* dict_off, int64_t nent,
                          const uint8_t* validity, const int64_t* pos,
                          int64_t nrows, int64_t* lens, int32_t* entry,
                          int32_t* status, hipStream_t stream) {
  if (nrows <= 0) return;
  int64_t blocks = (nrows + kThreads - 1) / kThreads;
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  hipLaunchKernelGGL(dict_str_lens_kernel, dim3((uint32_t)blocks), dim3(kThreads),
                     0, stream, idx, n_idx, dict_off, nent, validity, pos, nrows,
                     lens, entry, status);
}

void launch_dict_str_copy(const uint8_t* dict_bytes, int64_t dict_len,
                          const int64_t* dict_off, int64_t nent,
                          const int32_t* entry, const int64_t* row_off,
                          int64_t nrows, uint8_t* dst, int64_t total,
                          hipStream_t stream) {
  SegSrc s{dict_bytes, dict_len, dict_off, nent, entry};
  launch_seg_copy<true>(s, row_off, nrows, dst, total, stream);
}

}  // namespace lakesoul
