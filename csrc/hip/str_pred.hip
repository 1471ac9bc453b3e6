// String predicates on the GPU: one launch evaluates one leaf predicate
// (compare with a literal, membership in a sorted set, LIKE) over an
// offsets + bytes column and writes the bool mask, validity fused in. The
// per-row logic is ../cpp/str_pred.h, shared with the host twin.
//
// Two shapes:
//   rows : a thread per row. Short values: neighbouring lanes read the same
//          cache lines of `bytes`.
//   wave : a wave per row. Long values: the compare reads 64 x 8 bytes a
//          step and a ballot finds the first difference; a middle LIKE
//          segment is tried at 64 candidate starts a step and the lowest
//          matching lane wins.
// The operand is staged in LDS once per workgroup when it fits
// STR_PRED_LDS_BUDGET (16 KiB: eight 256-thread workgroups, the most a CU
// holds, then use 128 of its 160 KiB); a larger one, such as a big IN set,
// is read where it lies and stays in L2.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../cpp/str_pred.h"
#include "kernels.h"

namespace lakesoul {

#define SP_THREADS 256
#define SP_MAX_BLOCKS 2048

using lspred::Operand;

// eight bytes of p[pos .. pos + 8) as a big-endian word; bytes outside
// [0, n) read as 0
__device__ inline uint64_t load8_be(const uint8_t* p, int64_t pos, int64_t n) {
  if (pos >= 0 && pos + 8 <= n && (((uintptr_t)(p + pos)) & 7) == 0) {
    uint64_t x;
    __builtin_memcpy(&x, __builtin_assume_aligned(p + pos, 8), 8);
    return __builtin_bswap64(x);
  }
  uint64_t x = 0;
  for (int j = 0; j < 8; j++) {
    int64_t q = pos + j;
    uint8_t b = (q >= 0 && q < n) ? p[q] : 0;
    x = (x << 8) | b;
  }
  return x;
}

// lspred::compare by a whole wave: every lane gets the same result. Steps
// are laid on the 8-byte words of `a`, so its loads are whole words.
struct WaveCompare {
  __device__ int operator()(const uint8_t* a, int64_t alen, const uint8_t* b,
                            int64_t blen) const {
    const int lane = threadIdx.x & 63;
    int64_t n = alen < blen ? alen : blen;
    int64_t first = -(int64_t)((uintptr_t)a & 7);
    for (int64_t base = first; base < n; base += 512) {
      int64_t pos = base + lane * 8;
      int c = 0;
      if (pos < n) {
        uint64_t x = load8_be(a, pos, n), y = load8_be(b, pos, n);
        c = x == y ? 0 : x < y ? -1 : 1;
      }
      uint64_t diff = __ballot(c != 0);
      if (diff) return __shfl(c, __ffsll((unsigned long long)diff) - 1);
    }
    return alen == blen ? 0 : alen < blen ? -1 : 1;
  }
};

// lspred::SeqFind by a whole wave
struct WaveFind {
  __device__ int64_t operator()(const uint8_t* v, int64_t lo, int64_t hi,
                                const uint8_t* lit, const uint8_t* wild,
                                int64_t slen, bool utf8) const {
    const int lane = threadIdx.x & 63;
    for (int64_t base = lo; base + slen <= hi; base += 64) {
      int64_t pos = base + lane;
      long long e = -1;
      if (pos + slen <= hi && lspred::like_candidate(v, pos, utf8))
        e = lspred::seg_fwd(v, pos, hi, lit, wild, slen, utf8);
      uint64_t hit = __ballot(e >= 0);
      if (hit) return __shfl(e, __ffsll((unsigned long long)hit) - 1);
    }
    return -1;
  }
};

template <typename OffT, int WAVE>
__global__ __launch_bounds__(SP_THREADS) void str_pred_kernel(
    const OffT* __restrict__ offsets, const uint8_t* __restrict__ bytes,
    int64_t nbytes, const uint8_t* __restrict__ validity, int op,
    const uint8_t* __restrict__ op_bytes, int64_t op_nbytes,
    const int32_t* __restrict__ op_meta, int64_t op_nmeta, int in_lds,
    uint8_t* __restrict__ out, int64_t n) {
  extern __shared__ __attribute__((aligned(16))) uint8_t sp_lds[];
  Operand o{op_bytes, op_nbytes, op_meta, op_nmeta};
  if (in_lds) {
    // meta first (int32, at 0), the bytes behind it on a 16-byte boundary
    int64_t meta_bytes = (op_nmeta * 4 + 15) & ~(int64_t)15;
    int32_t* lm = (int32_t*)sp_lds;
    uint8_t* lb = sp_lds + meta_bytes;
    for (int64_t i = threadIdx.x; i < op_nmeta; i += SP_THREADS) lm[i] = op_meta[i];
    for (int64_t i = threadIdx.x; i < op_nbytes; i += SP_THREADS) lb[i] = op_bytes[i];
    __syncthreads();
    o.bytes = lb;
    o.meta = lm;
  }
  if constexpr (WAVE) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * SP_THREADS + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * SP_THREADS) >> 6;
    for (int64_t i = wave; i < n; i += nwaves) {
      bool r = false;
      if (!validity || validity[i]) {
        int64_t s, len;
        lspred::row_range(offsets, i, nbytes, s, len);
        r = lspred::row_pred(op, o, bytes + s, len, WaveCompare(), WaveFind());
      }
      if (lane == 0) out[i] = r ? 1 : 0;
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * SP_THREADS) {
      bool r = false;
      if (!validity || validity[i]) {
        int64_t s, len;
        lspred::row_range(offsets, i, nbytes, s, len);
        r = lspred::row_pred(op, o, bytes + s, len, lspred::SeqCompare(),
                             lspred::SeqFind());
      }
      out[i] = r ? 1 : 0;
    }
  }
}

int64_t str_pred_lds_budget() { return STR_PRED_LDS_BUDGET; }

template <typename OffT>
void launch_str_pred(const OffT* offsets, const uint8_t* bytes, int64_t nbytes,
                     const uint8_t* validity, int op, const uint8_t* op_bytes,
                     int64_t op_nbytes, const int32_t* op_meta,
                     int64_t op_nmeta, int wave_shape, uint8_t* out, int64_t n,
                     hipStream_t s) {
  if (n <= 0) return;
  int64_t lds = ((op_nmeta * 4 + 15) & ~(int64_t)15) + op_nbytes;
  int in_lds = lds <= STR_PRED_LDS_BUDGET;
  size_t shmem = in_lds ? (size_t)((lds + 15) & ~(int64_t)15) : 0;
  int64_t per_block = wave_shape ? SP_THREADS / 64 : SP_THREADS;
  int64_t blocks = (n + per_block - 1) / per_block;
  if (blocks > SP_MAX_BLOCKS) blocks = SP_MAX_BLOCKS;
  if (wave_shape)
    hipLaunchKernelGGL((str_pred_kernel<OffT, 1>), dim3((unsigned)blocks),
                       dim3(SP_THREADS), shmem, s, offsets, bytes, nbytes,
                       validity, op, op_bytes, op_nbytes, op_meta, op_nmeta,
                       in_lds, out, n);
  else
    hipLaunchKernelGGL((str_pred_kernel<OffT, 0>), dim3((unsigned)blocks),
                       dim3(SP_THREADS), shmem, s, offsets, bytes, nbytes,
                       validity, op, op_bytes, op_nbytes, op_meta, op_nmeta,
                       in_lds, out, n);
}

template void launch_str_pred<int32_t>(const int32_t*, const uint8_t*, int64_t,
                                       const uint8_t*, int, const uint8_t*,
                                       int64_t, const int32_t*, int64_t, int,
                                       uint8_t*, int64_t, hipStream_t);
template void launch_str_pred<int64_t>(const int64_t*, const uint8_t*, int64_t,
                                       const uint8_t*, int, const uint8_t*,
                                       int64_t, const int32_t*, int64_t, int,
                                       uint8_t*, int64_t, hipStream_t);

}  // namespace lakesoul
