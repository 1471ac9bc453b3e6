// gfx950 decoders for raw parquet value pages of a scan unit:
// DELTA_BINARY_PACKED and BYTE_STREAM_SPLIT. The host walks the serial
// headers (csrc/cpp/delta.h) and ships one table row per page and per
// miniblock (layout: csrc/cpp/read_unit.h, `enc`); the device does the
// per-value work. Every row's span was validated on the host against its
// page, and the payload region is padded by 8 bytes, so the unaligned
// 8-byte loads below stay inside the values buffer; `vals_len` is a last
// guard, not the contract.
//
// delta_binary_decode, two passes and a scan of one number per miniblock:
//   pass 1: one wave per miniblock. Lane j unpacks delta j, adds the
//           block's min_delta, the wave takes an inclusive scan (64 values
//           per step, a carry across steps) and writes the partial sums
//           and the miniblock's total.
//   scan  : inclusive cumsum of the totals (tiny: one int64 per miniblock).
//   pass 2: one wave per miniblock adds its base: the page's first value
//           plus the totals of the page's earlier miniblocks. One thread
//           per page writes the first value itself.
// All arithmetic is unsigned 64-bit and wraps; a 4-byte column keeps the
// low 32 bits, which is the same sum mod 2^32.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace lakesoul {

#define LSD_THREADS 256
#define LSD_WAVES (LSD_THREADS / 64)
#define LSD_MAX_BLOCKS 2048

// `width` (1..64) bits at absolute bit position `bitpos` of `payload`
__device__ inline uint64_t lsd_unpack(const uint8_t* __restrict__ payload,
                                      int64_t vals_len, uint64_t bitpos,
                                      int width) {
  uint64_t byte = bitpos >> 3;
  int ph = (int)(bitpos & 7);
  bool spill = ph + width > 64;  // widths 58..64 at a non-zero bit phase
  if ((int64_t)(byte + (spill ? 9 : 8)) > vals_len) return 0;
  uint64_t lo;
  __builtin_memcpy(&lo, payload + byte, 8);
  uint64_t v = lo >> ph;
  if (spill) v |= (uint64_t)payload[byte + 8] << (64 - ph);  // ph in 1..7
  return width >= 64 ? v : v & ((1ull << width) - 1);
}

template <typename T>
__global__ void delta_binary_pass1_kernel(const uint8_t* __restrict__ payload,
                                          int64_t vals_len,
                                          const int64_t* __restrict__ mbs,
                                          int64_t nmb, T* __restrict__ out,
                                          int64_t dense_n,
                                          int64_t* __restrict__ totals) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * LSD_WAVES;
  for (int64_t m = (int64_t)blockIdx.x * LSD_WAVES + (threadIdx.x >> 6);
       m < nmb; m += nwaves) {
    const int64_t* r = mbs + m * 6;  // wave-uniform
    const int64_t out_off = r[0], n = r[1];
    const uint64_t bit_off = (uint64_t)r[2];
    const int width = (int)r[3];
    const uint64_t min_delta = (uint64_t)r[4];
    uint64_t carry = 0;
    for (int64_t j0 = 0; j0 < n; j0 += 64) {
      int64_t j = j0 + lane;
      // lanes past n (the padding of a last miniblock) contribute 0
      uint64_t d = 0;
      if (j < n) {
        d = min_delta;
        if (width > 0)  // width 0: no payload, bit_off is not dereferenced
          d += lsd_unpack(payload, vals_len, bit_off + (uint64_t)j * width, width);
      }
      unsigned long long s = d;
      for (int off = 1; off < 64; off <<= 1) {
        unsigned long long t = __shfl_up(s, off, 64);
        if (lane >= off) s += t;
      }
      if (j < n && out_off + j < dense_n) out[out_off + j] = (T)(carry + s);
      carry += (uint64_t)__shfl(s, 63, 64);
    }
    if (lane == 0) totals[m] = (int64_t)carry;
  }
}

template <typename T>
__global__ void delta_binary_pass2_kernel(const int64_t* __restrict__ pages,
                                          int64_t npages,
                                          const int64_t* __restrict__ mbs,
                                          int64_t nmb,
                                          const int64_t* __restrict__ totals,
                                          const int64_t* __restrict__ csum,
                                          T* __restrict__ out, int64_t dense_n) {
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * LSD_WAVES;
  for (int64_t m = (int64_t)blockIdx.x * LSD_WAVES + (threadIdx.x >> 6);
       m < nmb; m += nwaves) {
    const int64_t* r = mbs + m * 6;
    const int64_t out_off = r[0], n = r[1];
    const int64_t* pg = pages + r[5] * 6;
    const int64_t m0 = pg[3];  // first miniblock of the page
    // first value + totals of the page's miniblocks before this one
    uint64_t base = (uint64_t)pg[2] +
                    ((uint64_t)csum[m] - (uint64_t)totals[m]) -
                    ((uint64_t)csum[m0] - (uint64_t)totals[m0]);
    for (int64_t j = lane; j < n; j += 64)
      if (out_off + j < dense_n) out[out_off + j] += (T)base;
  }
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < npages;
       p += (int64_t)gridDim.x * blockDim.x) {
    const int64_t* pg = pages + p * 6;
    if (pg[1] > 0 && pg[0] < dense_n) out[pg[0]] = (T)(uint64_t)pg[2];
  }
}

// thread per value: lane i reads byte k at page_off + k*n + i, so each of
// the ES loads is coalesced across the wave; assembled in registers,
// stored once. blockIdx.y strides the pages, blockIdx.x a page's values.
template <typename T>
__global__ void byte_stream_split_kernel(const uint8_t* __restrict__ payload,
                                         int64_t vals_len,
                                         const int64_t* __restrict__ pages,
                                         int64_t npages, T* __restrict__ out,
                                         int64_t dense_n) {
  constexpr int ES = (int)sizeof(T);
  for (int64_t p = blockIdx.y; p < npages; p += gridDim.y) {
    const int64_t* pg = pages + p * 6;
    const int64_t out_off = pg[0], n = pg[1], src_off = pg[2];
    if (n <= 0 || src_off < 0 || src_off + n * ES > vals_len ||
        out_off + n > dense_n)
      continue;
    const uint8_t* src = payload + src_off;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
      uint64_t v = 0;
#pragma unroll
      for (int k = 0; k < ES; k++) v |= (uint64_t)src[(int64_t)k * n + i] << (8 * k);
      out[out_off + i] = (T)v;
    }
  }
}

static inline int lsd_wave_blocks(int64_t nwaves) {
  int64_t b = (nwaves + LSD_WAVES - 1) / LSD_WAVES;
  if (b > LSD_MAX_BLOCKS) b = LSD_MAX_BLOCKS;
  if (b < 1) b = 1;
  return (int)b;
}

template <typename T>
void launch_delta_binary_pass1(const uint8_t* payload, int64_t vals_len,
                               const int64_t* mbs, int64_t nmb, T* out,
                               int64_t dense_n, int64_t* totals, hipStream_t s) {
  if (nmb <= 0) return;
  hipLaunchKernelGGL((delta_binary_pass1_kernel<T>), dim3(lsd_wave_blocks(nmb)),
                     dim3(LSD_THREADS), 0, s, payload, vals_len, mbs, nmb, out,
                     dense_n, totals);
}

template <typename T>
void launch_delta_binary_pass2(const int64_t* pages, int64_t npages,
                               const int64_t* mbs, int64_t nmb,
                               const int64_t* totals, const int64_t* csum, T* out,
                               int64_t dense_n, hipStream_t s) {
  if (npages <= 0) return;
  int64_t waves = nmb > (npages + 63) / 64 ? nmb : (npages + 63) / 64;
  hipLaunchKernelGGL((delta_binary_pass2_kernel<T>), dim3(lsd_wave_blocks(waves)),
                     dim3(LSD_THREADS), 0, s, pages, npages, mbs, nmb, totals,
                     csum, out, dense_n);
}

template <typename T>
void launch_byte_stream_split(const uint8_t* payload, int64_t vals_len,
                              const int64_t* pages, int64_t npages, T* out,
                              int64_t dense_n, hipStream_t s) {
  if (npages <= 0 || dense_n <= 0) return;
  // blocks along a page sized for the average page, pages along y, capped
  // like the other memory-bound kernels
  int64_t per_page = (dense_n + npages - 1) / npages;
  int64_t bx = (per_page + LSD_THREADS - 1) / LSD_THREADS;
  if (bx > LSD_MAX_BLOCKS) bx = LSD_MAX_BLOCKS;
  if (bx < 1) bx = 1;
  int64_t by = LSD_MAX_BLOCKS / bx;
  if (by > npages) by = npages;
  if (by < 1) by = 1;
  hipLaunchKernelGGL((byte_stream_split_kernel<T>), dim3((int)bx, (int)by),
                     dim3(LSD_THREADS), 0, s, payload, vals_len, pages, npages,
                     out, dense_n);
}

template void launch_delta_binary_pass1<uint32_t>(const uint8_t*, int64_t, const int64_t*, int64_t, uint32_t*, int64_t, int64_t*, hipStream_t);
template void launch_delta_binary_pass1<uint64_t>(const uint8_t*, int64_t, const int64_t*, int64_t, uint64_t*, int64_t, int64_t*, hipStream_t);
template void launch_delta_binary_pass2<uint32_t>(const int64_t*, int64_t, const int64_t*, int64_t, const int64_t*, const int64_t*, uint32_t*, int64_t, hipStream_t);
template void launch_delta_binary_pass2<uint64_t>(const int64_t*, int64_t, const int64_t*, int64_t, const int64_t*, const int64_t*, uint64_t*, int64_t, hipStream_t);
template void launch_byte_stream_split<uint32_t>(const uint8_t*, int64_t, const int64_t*, int64_t, uint32_t*, int64_t, hipStream_t);
template void launch_byte_stream_split<uint64_t>(const uint8_t*, int64_t, const int64_t*, int64_t, uint64_t*, int64_t, hipStream_t);

}  // namespace lakesoul
