// Parquet "v2" value encodings, parsed once: DELTA_BINARY_PACKED,
// DELTA_LENGTH_BYTE_ARRAY, DELTA_BYTE_ARRAY and BYTE_STREAM_SPLIT.
//
// delta_walk() is the one walk of a DELTA_BINARY_PACKED stream. It feeds
// the host decoder below and the miniblock table that drives the GPU
// kernel (read_unit.h -> csrc/hip/delta.hip), so both see the same
// validated spans: every miniblock it reports lies wholly inside the
// buffer, and no device address is ever derived from unvalidated bytes.
//
// Stream layout (parquet Encodings.md):
//   header : ULEB128 block_size, miniblocks_per_block, total_count;
//            zigzag first_value
//   block  : zigzag min_delta, one width byte per miniblock, then the
//            miniblocks, values_per_miniblock * width bits each
// The width bytes of a block are always all present; the payload of
// trailing miniblocks that carry no value is not. A partly filled last
// miniblock is padded to full size. All arithmetic is unsigned and wraps
// (mod 2^64; an INT32 column truncates to mod 2^32).
#pragma once

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <type_traits>
#include <vector>

namespace lakesoul {

struct DeltaHeader {
  uint64_t block_size = 0;
  uint64_t miniblocks = 0;          // per block
  uint64_t values_per_miniblock = 0;
  uint64_t count = 0;               // values in the stream, first included
  uint64_t first_value = 0;
};

struct DeltaMiniblock {
  int64_t first;       // index in the page of the first value it produces (>= 1)
  int64_t n;           // values it carries (<= values_per_miniblock)
  int64_t bit_off;     // absolute bit offset of its payload in the stream
  int32_t bit_width;   // 0..type_bits; 0 = no payload
  uint64_t min_delta;  // of its block
};

namespace delta_detail {

inline uint64_t uleb128(const uint8_t* p, size_t len, size_t& pos) {
  uint64_t v = 0;
  for (int shift = 0; shift < 70; shift += 7) {
    if (pos >= len) throw std::runtime_error("delta: truncated varint");
    uint8_t b = p[pos++];
    if (shift == 63 && (b & 0x7E)) throw std::runtime_error("delta: varint overflow");
    v |= (uint64_t)(b & 0x7F) << shift;
    if (!(b & 0x80)) return v;
  }
  throw std::runtime_error("delta: varint too long");
}

inline uint64_t zigzag(uint64_t v) { return (v >> 1) ^ (~(v & 1) + 1); }

// `width` bits at absolute bit position `bit`; the caller has validated
// that [bit, bit + width) lies inside p[0, len)
inline uint64_t unpack_bits(const uint8_t* p, size_t len, uint64_t bit, int width) {
  size_t byte = (size_t)(bit >> 3);
  int ph = (int)(bit & 7);
  uint64_t v;
  if (byte + 9 <= len) {
    uint64_t lo;
    std::memcpy(&lo, p + byte, 8);
    v = lo >> ph;
    if (ph + width > 64) v |= (uint64_t)p[byte + 8] << (64 - ph);
  } else {
    v = 0;
    int got = 0;
    while (got < width) {
      uint64_t b = (uint64_t)p[byte++] >> ph;
      v |= b << got;  // bits past `width` are masked below
      got += 8 - ph;
      ph = 0;
    }
  }
  return width >= 64 ? v : v & ((1ull << width) - 1);
}

}  // namespace delta_detail

// Walk one DELTA_BINARY_PACKED stream of a `type_bits` (32 or 64) wide
// column that may hold at most `max_count` values. Calls
// on_miniblock(const DeltaMiniblock&) for every miniblock that carries
// values, in stream order, and returns the bytes the stream occupies.
// Throws std::runtime_error on anything malformed or out of bounds.
template <typename F>
inline size_t delta_walk(const uint8_t* p, size_t len, int type_bits,
                         uint64_t max_count, DeltaHeader& h, F&& on_miniblock) {
  using namespace delta_detail;
  size_t pos = 0;
  h.block_size = uleb128(p, len, pos);
  h.miniblocks = uleb128(p, len, pos);
  h.count = uleb128(p, len, pos);
  h.first_value = zigzag(uleb128(p, len, pos));
  if (h.block_size == 0 || h.block_size % 128 != 0 || h.block_size > (1u << 24))
    throw std::runtime_error("delta: bad block size");
  if (h.miniblocks == 0 || h.block_size % h.miniblocks != 0)
    throw std::runtime_error("delta: bad miniblock count");
  h.values_per_miniblock = h.block_size / h.miniblocks;
  if (h.values_per_miniblock % 32 != 0)
    throw std::runtime_error("delta: miniblock size not a multiple of 32");
  if (h.count > max_count)
    throw std::runtime_error("delta: stream holds more values than the page");
  const uint64_t vpm = h.values_per_miniblock;
  uint64_t remaining = h.count ? h.count - 1 : 0;
  int64_t idx = 1;
  while (remaining > 0) {
    uint64_t min_delta = zigzag(uleb128(p, len, pos));
    if (h.miniblocks > len - pos)
      throw std::runtime_error("delta: truncated miniblock widths");
    const uint8_t* widths = p + pos;
    pos += (size_t)h.miniblocks;
    for (uint64_t mb = 0; mb < h.miniblocks && remaining > 0; mb++) {
      int w = widths[mb];
      if (w > type_bits) throw std::runtime_error("delta: bit width too large");
      uint64_t bytes = vpm * (uint64_t)w / 8;  // vpm % 32 == 0: exact
      if (bytes > len - pos)
        throw std::runtime_error("delta: miniblock past the end of the page");
      DeltaMiniblock m;
      m.first = idx;
      m.n = (int64_t)(remaining < vpm ? remaining : vpm);
      m.bit_off = (int64_t)pos * 8;
      m.bit_width = w;
      m.min_delta = min_delta;
      on_miniblock(m);
      pos += (size_t)bytes;
      idx += m.n;
      remaining -= (uint64_t)m.n;
    }
  }
  return pos;
}

// Decode a stream of exactly `n` values of T (int32_t / int64_t), appended
// to `out` as raw little-endian values. Returns the bytes consumed.
template <typename T>
inline size_t delta_binary_decode(const uint8_t* p, size_t len, int64_t n,
                                  std::vector<uint8_t>& out) {
  using U = typename std::make_unsigned<T>::type;
  if (n <= 0) return 0;
  size_t base = out.size();
  // out grows as values decode, never from the header's claim alone
  uint64_t cur = 0;
  int64_t produced = 0;
  auto emit = [&](uint64_t v) {
    U t = (U)v;
    size_t at = out.size();
    out.resize(at + sizeof(U));
    std::memcpy(out.data() + at, &t, sizeof(U));
    produced++;
  };
  DeltaHeader h;
  bool first_done = false;
  size_t used = delta_walk(p, len, (int)sizeof(T) * 8, (uint64_t)n, h,
                           [&](const DeltaMiniblock& m) {
    if (!first_done) {
      cur = h.first_value;
      emit(cur);
      first_done = true;
    }
    for (int64_t j = 0; j < m.n; j++) {
      uint64_t d = m.bit_width
                       ? delta_detail::unpack_bits(
                             p, len, (uint64_t)m.bit_off + (uint64_t)j * m.bit_width,
                             m.bit_width)
                       : 0;
      cur += m.min_delta + d;
      emit(cur);
    }
  });
  if (!first_done && h.count) emit(h.first_value);
  if (produced != n) {
    out.resize(base);
    throw std::runtime_error("delta: stream holds fewer values than the page");
  }
  return used;
}

// DELTA_LENGTH_BYTE_ARRAY: `n` lengths as a DELTA_BINARY_PACKED stream,
// then the concatenated bytes. Appends the PLAIN form ((u32 len, bytes)
// per value) to `out`; returns the bytes consumed.
inline size_t delta_length_byte_array_decode(const uint8_t* p, size_t len,
                                             int64_t n, std::vector<uint8_t>& out) {
  if (n <= 0) return 0;
  std::vector<uint8_t> lens_raw;
  size_t pos = delta_binary_decode<int32_t>(p, len, n, lens_raw);
  for (int64_t i = 0; i < n; i++) {
    int32_t l;
    std::memcpy(&l, lens_raw.data() + i * 4, 4);
    if (l < 0 || (size_t)l > len - pos)
      throw std::runtime_error("delta-length: value past the end of the page");
    uint32_t ul = (uint32_t)l;
    size_t at = out.size();
    out.resize(at + 4 + ul);
    std::memcpy(out.data() + at, &ul, 4);
    if (ul) std::memcpy(out.data() + at + 4, p + pos, ul);
    pos += ul;
  }
  return pos;
}

// DELTA_BYTE_ARRAY: prefix lengths (DELTA_BINARY_PACKED), then suffixes
// (DELTA_LENGTH_BYTE_ARRAY). A value is the previous value's prefix plus
// its suffix; the first value of a page has no previous value. Appends
// the PLAIN form to `out`; returns the bytes consumed.
inline size_t delta_byte_array_decode(const uint8_t* p, size_t len, int64_t n,
                                      std::vector<uint8_t>& out) {
  if (n <= 0) return 0;
  std::vector<uint8_t> pre_raw, suf_raw;
  size_t pos = delta_binary_decode<int32_t>(p, len, n, pre_raw);
  pos += delta_binary_decode<int32_t>(p + pos, len - pos, n, suf_raw);
  size_t prev_at = 0;   // previous value's bytes inside `out`
  uint32_t prev_len = 0;
  for (int64_t i = 0; i < n; i++) {
    int32_t pre, suf;
    std::memcpy(&pre, pre_raw.data() + i * 4, 4);
    std::memcpy(&suf, suf_raw.data() + i * 4, 4);
    if (pre < 0 || (uint32_t)pre > prev_len)
      throw std::runtime_error("delta-byte-array: prefix longer than the previous value");
    if (suf < 0 || (size_t)suf > len - pos)
      throw std::runtime_error("delta-byte-array: suffix past the end of the page");
    uint64_t total = (uint64_t)pre + (uint64_t)suf;
    if (total > 0x7FFFFFFFull)
      throw std::runtime_error("delta-byte-array: value too long");
    uint32_t ul = (uint32_t)total;
    size_t at = out.size();
    out.resize(at + 4 + ul);  // may move the previous value: index, not pointer
    std::memcpy(out.data() + at, &ul, 4);
    if (pre) std::memmove(out.data() + at + 4, out.data() + prev_at, (size_t)pre);
    if (suf) std::memcpy(out.data() + at + 4 + pre, p + pos, (size_t)suf);
    pos += (size_t)suf;
    prev_at = at + 4;
    prev_len = ul;
  }
  return pos;
}

// BYTE_STREAM_SPLIT: byte k of value i sits at k*n + i, n = the page's
// stored value count. Appends n values of `es` bytes to `out`.
inline void byte_stream_split_decode(const uint8_t* p, size_t len, int64_t n,
                                     int es, std::vector<uint8_t>& out) {
  if (n <= 0) return;
  if ((uint64_t)n > len / (uint64_t)es)
    throw std::runtime_error("byte-stream-split: page shorter than its values");
  size_t at = out.size();
  out.resize(at + (size_t)n * es);
  uint8_t* o = out.data() + at;
  for (int k = 0; k < es; k++) {
    const uint8_t* s = p + (size_t)k * n;
    for (int64_t i = 0; i < n; i++) o[i * es + k] = s[i];
  }
}

}  // namespace lakesoul
