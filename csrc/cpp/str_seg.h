// Segment copy, the locate step: a string column is a run of segments
// (values) laid end to end in the output; `off` holds nseg + 1 int64
// destination offsets, off[0] = 0, non-decreasing. The functions here say
// which segment owns an output byte and where that byte comes from. They are
// shared by the GPU kernel (csrc/hip/strings.hip) and its host twins at the
// end of this file, which the CPU tests and the sanitizer program
// (tests/str_walk_san.cc) run.
//
// Two sources:
//   prefix strip : the PLAIN stream (u32 len, bytes)*: byte b of the output,
//                  owned by value i, sits at raw[b + 4 * (i + 1)]
//   dictionary   : value i is entry k = entry_of[i] of a dictionary whose
//                  stripped bytes are dict_bytes and whose entry k spans
//                  dict_off[k] .. dict_off[k + 1]: byte b sits at
//                  dict_bytes[dict_off[k] + (b - off[i])]
#pragma once

#include <cstddef>
#include <cstdint>

#ifndef LSSEG_HD
#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#define LSSEG_HD __host__ __device__
#else
#define LSSEG_HD
#endif
#endif

namespace lsseg {

// first j in [lo, hi) with off[j] > b; hi when there is none
LSSEG_HD inline int64_t upper_bound(const int64_t* off, int64_t lo, int64_t hi,
                                    int64_t b) {
  while (lo < hi) {
    int64_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] > b) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// The segment that owns byte b, looked for among segments lo .. nseg - 1:
// the last one that starts at or before b, so a run of empty segments in
// front of it is skipped, not visited. The caller knows off[lo] <= b. The
// result is in [lo, nseg - 1] whatever the table holds.
LSSEG_HD inline int64_t owner(const int64_t* off, int64_t lo, int64_t nseg,
                              int64_t b) {
  return upper_bound(off, lo + 1, nseg, b) - 1;
}

// source index minus output index for the bytes of segment i
LSSEG_HD inline int64_t strip_delta(int64_t i) { return 4 * (i + 1); }

// dictionary entry k of a value that starts at output offset seg_start;
// false when k is no entry (the value then has no bytes)
LSSEG_HD inline bool dict_delta(const int64_t* dict_off, int64_t nent, int64_t k,
                                int64_t seg_start, int64_t& delta) {
  if (k < 0 || k >= nent) return false;
  delta = dict_off[k] - seg_start;
  return true;
}

// length of the value that row r of a dictionary column holds, and its
// entry: 0 and -1 for a null row; 0, -1 and a status bit for an index that
// is no entry (1) or a row with no stored index (2)
LSSEG_HD inline int64_t dict_row_len(const int32_t* idx, int64_t n_idx,
                                     const int64_t* dict_off, int64_t nent,
                                     bool valid, int64_t dense_pos,
                                     int32_t& entry, int32_t& status) {
  entry = -1;
  status = 0;
  if (!valid) return 0;
  if (dense_pos < 0 || dense_pos >= n_idx) {
    status = 2;
    return 0;
  }
  int64_t k = idx[dense_pos];
  if (k < 0 || k >= nent) {
    status = 1;
    return 0;
  }
  int64_t len = dict_off[k + 1] - dict_off[k];
  if (len < 0) {
    status = 1;
    return 0;
  }
  entry = (int32_t)k;
  return len;
}

}  // namespace lsseg

#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>

namespace lsseg {

// Host twin of the segment copy: every output byte through the same locate
// functions as the kernel. src_len bounds every read; a byte whose source
// lies outside reads as 0. entry_of == nullptr: prefix strip.
inline void seg_copy_host(const uint8_t* src, int64_t src_len,
                          const int64_t* dict_off, int64_t nent,
                          const int32_t* entry_of, const int64_t* off,
                          int64_t nseg, uint8_t* dst, int64_t total) {
  if (total <= 0 || nseg <= 0) return;
  int64_t seg = -1, seg_end = 0, delta = 0;
  bool have = false;
  for (int64_t b = 0; b < total; b++) {
    if (seg < 0 || b >= seg_end) {
      seg = owner(off, seg < 0 ? 0 : seg, nseg, b);
      seg_end = off[seg + 1];
      if (entry_of) {
        have = dict_delta(dict_off, nent, entry_of[seg], off[seg], delta);
      } else {
        have = true;
        delta = strip_delta(seg);
      }
    }
    int64_t si = b + delta;
    dst[b] = have && si >= 0 && si < src_len ? src[si] : 0;
  }
}

// strip_prefixes twin: raw PLAIN stream + dense offsets -> compact bytes
inline std::vector<uint8_t> strip_prefixes_host(const uint8_t* raw,
                                                int64_t raw_len,
                                                const int64_t* doff,
                                                int64_t n) {
  int64_t total = n > 0 ? doff[n] : 0;
  std::vector<uint8_t> out((size_t)(total > 0 ? total : 0));
  seg_copy_host(raw, raw_len, nullptr, 0, nullptr, doff, n, out.data(), total);
  return out;
}

// dict_strings twin: dense indices (+ optional row validity) -> row offsets
// (nrows + 1), compact bytes, status
inline int32_t dict_strings_host(const int32_t* idx, int64_t n_idx,
                                 const int64_t* dict_off, int64_t nent,
                                 const uint8_t* dict_bytes, int64_t dict_len,
                                 const uint8_t* validity, int64_t nrows,
                                 std::vector<int64_t>& offsets,
                                 std::vector<uint8_t>& bytes) {
  offsets.assign((size_t)nrows + 1, 0);
  std::vector<int32_t> entry((size_t)nrows);
  int32_t status = 0;
  int64_t dense = 0;
  for (int64_t r = 0; r < nrows; r++) {
    bool valid = !validity || validity[r];
    int32_t st;
    int64_t len = dict_row_len(idx, n_idx, dict_off, nent, valid, dense,
                               entry[(size_t)r], st);
    status |= st;
    if (valid) dense++;
    offsets[(size_t)r + 1] = offsets[(size_t)r] + len;
  }
  bytes.assign((size_t)offsets[(size_t)nrows], 0);
  seg_copy_host(dict_bytes, dict_len, dict_off, nent, entry.data(),
                offsets.data(), nrows, bytes.data(), offsets[(size_t)nrows]);
  return status;
}

}  // namespace lsseg
#endif
