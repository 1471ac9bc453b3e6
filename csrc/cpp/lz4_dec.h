// LZ4 block format, written from the format description
// (lz4_Block_format.md): the sequence parser and the block decoder are
// shared by the host (parquet codecs 7 LZ4_RAW and 5 LZ4 with Hadoop
// framing, compress.h) and the GPU kernel (csrc/hip/lz4.hip), which calls
// lz4_parse_seq on every lane and does the byte movement itself. The
// encoder at the end is host-only.
//
// A block is a run of sequences:
//   token            high nibble: literal length, low nibble: match length-4
//   [ext bytes]      when the literal nibble is 15: add bytes until one < 255
//   literals
//   offset           2 bytes little-endian, 1..65535, back from the output
//   [ext bytes]      when the match nibble is 15
// The last sequence stops after its literals.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#ifndef LSL4_HD
#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#define LSL4_HD __host__ __device__
#else
#define LSL4_HD
#endif
#endif

namespace lslz4 {

struct Seq {
  int64_t lit_pos;     // first literal byte in src
  uint64_t lit_len;
  bool last;           // the literals end the block: no match part
  uint32_t offset;
  uint64_t match_len;
  int64_t next;        // where the next sequence starts
};

// length nibble + extension bytes at src[pos..): every read is checked
// against n; the sum is 64-bit and each byte adds at most 255, so it
// cannot wrap for any n that fits memory
LSL4_HD inline bool read_len_ext(const uint8_t* src, int64_t n, int64_t& pos,
                                 uint64_t& len) {
  if (len != 15) return true;
  uint8_t b;
  do {
    if (pos >= n) return false;
    b = src[pos++];
    len += b;
  } while (b == 255);
  return true;
}

// One sequence header at src[pos]. False when it runs past src + n. A
// sequence whose literals reach src + n exactly is the last one; the match
// nibble of its token is not looked at (liblz4 does the same).
LSL4_HD inline bool lz4_parse_seq(const uint8_t* src, int64_t n, int64_t pos,
                              Seq& q) {
  if (pos < 0 || pos >= n) return false;
  uint8_t token = src[pos++];
  q.lit_len = token >> 4;
  if (!read_len_ext(src, n, pos, q.lit_len)) return false;
  q.lit_pos = pos;
  if (q.lit_len > (uint64_t)(n - pos)) return false;
  pos += (int64_t)q.lit_len;
  q.last = pos == n;
  q.offset = 0;
  q.match_len = 0;
  q.next = pos;
  if (q.last) return true;
  if (n - pos < 2) return false;
  q.offset = (uint32_t)src[pos] | ((uint32_t)src[pos + 1] << 8);
  pos += 2;
  q.match_len = token & 15;
  if (!read_len_ext(src, n, pos, q.match_len)) return false;
  q.match_len += 4;
  q.next = pos;
  return true;
}

// Decode one block of exactly src_n bytes into exactly dst_n bytes. Reads
// only [src, src + src_n), writes only [dst, dst + dst_n). A block that
// ends with a match fails: the parse at src + src_n finds no token.
LSL4_HD inline bool lz4_block_decode(uint8_t* dst, int64_t dst_n,
                                 const uint8_t* src, int64_t src_n) {
  if (dst_n < 0) return false;
  int64_t pos = 0, d = 0;
  for (;;) {
    Seq q;
    if (!lz4_parse_seq(src, src_n, pos, q)) return false;
    if (q.lit_len > (uint64_t)(dst_n - d)) return false;
    for (uint64_t i = 0; i < q.lit_len; i++) dst[d + i] = src[q.lit_pos + i];
    d += (int64_t)q.lit_len;
    if (q.last) return d == dst_n;
    if (q.offset == 0 || (int64_t)q.offset > d) return false;
    if (q.match_len > (uint64_t)(dst_n - d)) return false;
    const uint8_t* from = dst + d - q.offset;
    for (uint64_t i = 0; i < q.match_len; i++) dst[d + i] = from[i];  // may overlap
    d += (int64_t)q.match_len;
    pos = q.next;
  }
}

LSL4_HD inline uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) |
         ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

// Parquet codec 5: Hadoop frames, each [u32 BE uncompressed size]
// [u32 BE compressed size][block]. Writers that never framed (old
// parquet-cpp) put one raw block there, so the frames are taken only when
// their sizes add up to dst_n and src_n exactly and every block decodes;
// otherwise the body is one raw block.
inline bool lz4_hadoop_decode(uint8_t* dst, int64_t dst_n, const uint8_t* src,
                          int64_t src_n) {
  if (dst_n < 0) return false;
  bool framed = true;
  int64_t pos = 0, d = 0;
  while (pos < src_n) {
    if (src_n - pos < 8) { framed = false; break; }
    int64_t u = be32(src + pos), c = be32(src + pos + 4);
    pos += 8;
    if (c > src_n - pos || u > dst_n - d) { framed = false; break; }
    pos += c;
    d += u;
  }
  if (framed && d == dst_n) {
    pos = 0;
    d = 0;
    while (pos < src_n) {
      int64_t u = be32(src + pos), c = be32(src + pos + 4);
      pos += 8;
      if (!lz4_block_decode(dst + d, u, src + pos, c)) { framed = false; break; }
      pos += c;
      d += u;
    }
    if (framed) return true;
  }
  return lz4_block_decode(dst, dst_n, src, src_n);
}

}  // namespace lslz4

#if !defined(__HIP_DEVICE_COMPILE__)
#include <stdexcept>
#include <vector>

namespace lslz4 {

inline void put_len_ext(std::vector<uint8_t>& out, size_t rest) {
  while (rest >= 255) {
    out.push_back(255);
    rest -= 255;
  }
  out.push_back((uint8_t)rest);
}

inline void put_seq(std::vector<uint8_t>& out, const uint8_t* lit, size_t ll,
                    size_t offset, size_t ml) {  // ml == 0: last sequence
  size_t mn = ml ? ml - 4 : 0;
  out.push_back((uint8_t)(((ll < 15 ? ll : 15) << 4) | (mn < 15 ? mn : 15)));
  if (ll >= 15) put_len_ext(out, ll - 15);
  out.insert(out.end(), lit, lit + ll);
  if (!ml) return;
  out.push_back((uint8_t)(offset & 255));
  out.push_back((uint8_t)(offset >> 8));
  if (mn >= 15) put_len_ext(out, mn - 15);
}

// Greedy single-pass encoder over a hash table of 4-byte prefixes. It keeps
// the format's end-of-block rules, which other decoders rely on: the last
// 5 bytes are literals, the last match starts at least 12 bytes before the
// end, so an input under 13 bytes is one literal run. Misses step faster
// the longer they last, so incompressible pages cost one probe per few
// bytes.
inline std::vector<uint8_t> lz4_block_encode(const uint8_t* src, size_t n) {
  if (n > 0x7E000000u) throw std::runtime_error("lz4: block too large");
  std::vector<uint8_t> out;
  out.reserve(n + n / 255 + 16);
  const int kHashBits = 13;
  std::vector<int32_t> table((size_t)1 << kHashBits, -1);
  auto rd32 = [&](size_t i) {
    uint32_t v;
    std::memcpy(&v, src + i, 4);
    return v;
  };
  size_t anchor = 0;
  if (n >= 13) {
    const size_t last_start = n - 12;  // a match may start here at the latest
    const size_t match_end = n - 5;    // and must end here at the latest
    size_t i = 0, miss = 0;
    while (i <= last_start) {
      uint32_t v = rd32(i);
      uint32_t h = (v * 2654435761u) >> (32 - kHashBits);
      int32_t cand = table[h];
      table[h] = (int32_t)i;
      if (cand >= 0 && i - (size_t)cand <= 65535 && rd32((size_t)cand) == v) {
        size_t ml = 4;
        while (i + ml < match_end && src[cand + ml] == src[i + ml]) ml++;
        put_seq(out, src + anchor, i - anchor, i - (size_t)cand, ml);
        i += ml;
        anchor = i;
        miss = 0;
      } else {
        i += 1 + (miss++ >> 6);
      }
    }
  }
  put_seq(out, src + anchor, n - anchor, 0, 0);
  return out;
}

}  // namespace lslz4
#endif
