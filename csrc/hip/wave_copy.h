// Byte movement of the one-wave-per-page decompressors (zstd.hip, lz4.hip):
// all 64 lanes of the wave copy one segment. Bytes that other lanes of the
// wave stored earlier are read through volatile (GLC) loads, and
// s_waitcnt(0) after a cooperative segment orders its stores before those
// reads (the snappy kernel's pattern).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lswave {

static const int kLanes = 64;

__device__ inline void waitcnt0() { __builtin_amdgcn_s_waitcnt(0); }

// unaligned-capable wide element copy: 8 bytes per lane per iteration
// (gfx950 flat loads support byte-aligned addresses), byte tail
template <bool VOL>
__device__ inline void wcopy_wide(uint8_t* dst, const uint8_t* src,
                                  int64_t len, int lane) {
  int64_t n8 = len >> 3;
  for (int64_t j = lane; j < n8; j += kLanes) {
    uint64_t w;
    if (VOL)
      w = *(const volatile uint64_t*)(src + 8 * j);
    else
      __builtin_memcpy(&w, src + 8 * j, 8);
    *(uint64_t*)(dst + 8 * j) = w;
  }
  for (int64_t j = (n8 << 3) + lane; j < len; j += kLanes)
    dst[j] = VOL ? ((volatile const uint8_t*)src)[j] : src[j];
}

// cooperative (possibly overlapping) match copy inside dst
__device__ inline void wcopy_match(uint8_t* base, int64_t out, uint32_t offset,
                                   uint32_t len, int lane) {
  for (uint32_t j = lane; j < len; j += kLanes) {
    uint32_t sj = (offset >= len) ? j : (j % offset);
    base[out + j] = ((volatile const uint8_t*)base)[out - offset + sj];
  }
  waitcnt0();
}

// cooperative copy from the (read-only) compressed input
__device__ inline void wcopy_src(uint8_t* dst, const uint8_t* src,
                                 int64_t len, int lane) {
  wcopy_wide<false>(dst, src, len, lane);
  waitcnt0();
}

}  // namespace lswave
