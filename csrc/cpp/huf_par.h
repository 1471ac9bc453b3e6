// Lane-parallel decode of one zstd Huffman stream (after Weissenberger and
// Schmidt, "Massively Parallel Huffman Decoding on GPUs", ICPP 2018).
//
// A Huffman stream is a dependent chain: where a codeword starts is known
// only once the one before it is decoded. But Huffman codes
// self-synchronise: a decoder started at an arbitrary bit falls onto true
// codeword boundaries after a short run (tens of bits on real column
// bytes). So the stream is cut into L sub-sequences, one per lane:
//
//   pass 1   every lane decodes from its own cut to the next one and notes
//            where it left (its exit) and how many codewords began inside
//            its range. Lane 0 starts at the stream's end mark, so it is
//            right.
//   fix-up   lane i+1's true start is lane i's exit. Every lane whose
//            predecessor's exit differs from the start it last used decodes
//            again from there, until no lane changed: at most L rounds
//            (lanes 0..k are right after round k), one or two on real data,
//            all L for equal-length codes whose cuts fall inside a codeword.
//   write    an exclusive prefix sum of the counts gives every lane its
//            output offset; it decodes once more and stores its symbols,
//            packed into aligned 8-byte words.
//
// The stream is valid only if the counts sum to its expected length and
// the last lane exits exactly at the stream's first bit; nothing is written
// otherwise.
//
// Positions here are bit indices `b` from the stream's FIRST bit: zstd
// streams are read backwards from the end mark, so a lane that has consumed
// p bits of a T-bit stream stands at b = T - p. Lane i of L owns
// b in (T - (i+1)S, T - iS], S = ceil(T / L). Bits below 0 read as zero; a
// lane never takes more steps than it owns bits, so no input can make it
// loop or leave its range by more than one codeword.
//
// The per-lane steps are LSZ_HD and run unchanged in the kernel
// (csrc/hip/zstd_huf.hip, one workgroup per stream, lanes = 256) and in
// the host twin at the end of this file (a loop over lanes), which is the
// kernel's reference and runs under the sanitizers
// (csrc/cpp/tests/huf_par_san.cc).
#pragma once

#include "zstd_dec.h"

namespace lszstd {

// bits of a backward stream below its end mark, -1 without a mark
LSZ_HD inline int32_t huf_stream_bits(const uint8_t* src, int64_t n) {
  if (n <= 0 || n > (1 << 20) || src[n - 1] == 0) return -1;
  return (int32_t)(n - 1) * 8 + highbit32(src[n - 1]);
}

// cut width for L lanes
LSZ_HD inline int32_t huf_lane_span(int32_t T, int lanes) {
  int32_t s = (T + lanes - 1) / lanes;
  return s < 1 ? 1 : s;
}

// lane i's range (bTop, bEnd]: it decodes while b > bEnd
LSZ_HD inline int32_t huf_lane_top(int32_t T, int32_t S, int i) {
  int64_t p = (int64_t)i * S;
  return p >= T ? 0 : T - (int32_t)p;
}

// 64-bit register window over the stream, read downwards
struct HufWin {
  const uint8_t* src;
  uint64_t win;   // stream bits [base, base + 64)
  int32_t base;   // multiple of 8, may be negative: those bits are zero

  // window whose top byte holds bit b - 1. Reads src[0 .. ceil(b / 8))
  // only: never past the byte that holds the end mark.
  LSZ_HD void refill(int32_t b) {
    int32_t top = (b + 7) >> 3;  // arithmetic shift: b may be below zero
    base = top * 8 - 64;
    if (top >= 8) {
      memcpy(&win, src + top - 8, 8);
    } else {
      uint64_t w = 0;
      for (int32_t k = 0; k < top; k++) w |= (uint64_t)src[k] << (8 * (8 - top + k));
      win = w;
    }
  }

  // bits [b - nb, b), nb <= 11
  LSZ_HD uint32_t peek(int32_t b, int nb) {
    int32_t sh = b - nb - base;
    if (sh < 0) {
      refill(b);
      sh = b - nb - base;
    }
    return (uint32_t)(win >> sh) & ((1u << nb) - 1);
  }
};

struct HufLaneExit {
  int32_t b;      // where the lane left: first codeword of the next lane
  int32_t count;  // codewords that began in (bEnd, bStart]
};

// passes 1 and fix-up: decode from bStart while b > bEnd, store nothing
LSZ_HD inline HufLaneExit huf_lane_scan(const HufTable& t, const uint8_t* src,
                                        int32_t bStart, int32_t bEnd) {
  HufLaneExit r{bStart, 0};
  if (bStart <= bEnd) return r;
  const int mb = t.maxBits;
  HufWin w{src, 0, 0};
  w.refill(bStart);
  int32_t b = bStart;
  int32_t n = 0;
  while (b > bEnd) {  // at most bStart - bEnd steps: each takes >= 1 bit
    uint32_t nb = t.e[w.peek(b, mb)].nbBits;
    b -= (int32_t)(nb ? nb : 1);
    n++;
  }
  r.b = b;
  r.count = n;
  return r;
}

// one aligned 8-byte word of output under construction
struct HufPack {
  uint8_t* word;  // 8-byte aligned
  uint64_t acc;
  int lo, hi;     // bytes [lo, hi) of the word are this lane's

  LSZ_HD void open(uint8_t* dst) {
    lo = hi = (int)((uintptr_t)dst & 7);
    word = dst - lo;
    acc = 0;
  }
  LSZ_HD void flush() {
    if (lo == 0 && hi == 8) {
      memcpy(word, &acc, 8);  // aligned: one store
    } else {
      for (int k = lo; k < hi; k++) word[k] = (uint8_t)(acc >> (8 * k));
    }
    word += 8;
    acc = 0;
    lo = hi = 0;
  }
  LSZ_HD void put(uint8_t v) {
    acc |= (uint64_t)v << (8 * hi);
    if (++hi == 8) flush();
  }
  LSZ_HD void close() {
    if (hi > lo) flush();
  }
};

// write pass: decode `count` codewords from bStart into dst[0 .. count)
LSZ_HD inline void huf_lane_write(const HufTable& t, const uint8_t* src,
                                  int32_t bStart, int32_t count, uint8_t* dst) {
  if (count <= 0) return;
  const int mb = t.maxBits;
  HufWin w{src, 0, 0};
  w.refill(bStart);
  HufPack out;
  out.open(dst);
  int32_t b = bStart;
  for (int32_t i = 0; i < count; i++) {
    HufEntry e = t.e[w.peek(b, mb)];
    out.put(e.symbol);
    b -= (int32_t)(e.nbBits ? e.nbBits : 1);
  }
  out.close();
}

// stream `i` of a Huffman-only page's payload after its tree description:
// p[0 .. rem). Checks the stream's place, end mark and output slice.
struct HufParStream {
  const uint8_t* src;
  int32_t T;
  int64_t outStart, outLen;
};

LSZ_HD inline bool huf_par_stream(const uint8_t* p, int64_t rem, int64_t rs,
                                  int nStreams, int i, HufParStream& s) {
  if (nStreams == 1) {
    s.src = p;
    s.outStart = 0;
    s.outLen = rs;
    s.T = huf_stream_bits(p, rem);
  } else {
    HufStream h;
    if (!huf4_stream(p, rem, rs, i, h)) return false;
    s.src = p + h.start;
    s.outStart = h.outStart;
    s.outLen = h.outLen;
    s.T = huf_stream_bits(s.src, h.len);
  }
  return s.T >= 0;
}

// ---------------------------------------------------------------------- //
// host twin: the same steps, a loop where the device has lanes
// ---------------------------------------------------------------------- //

static const int kHufParMaxLanes = 256;

struct HufParCtx {
  HufTable huf;
  BuildWs ws;
  int32_t start[kHufParMaxLanes], exitb[kHufParMaxLanes],
      prev[kHufParMaxLanes], count[kHufParMaxLanes];
  int rounds;  // most fix-up rounds any stream of the last page took
};

inline bool huf_par_stream_host(HufParCtx& c, const HufParStream& s,
                                uint8_t* dst, int lanes) {
  const int32_t S = huf_lane_span(s.T, lanes);
  for (int i = 0; i < lanes; i++) {
    c.start[i] = huf_lane_top(s.T, S, i);
    HufLaneExit r =
        huf_lane_scan(c.huf, s.src, c.start[i], huf_lane_top(s.T, S, i + 1));
    c.exitb[i] = r.b;
    c.count[i] = r.count;
  }
  int rounds = 0;
  for (;; rounds++) {
    if (rounds > lanes) return false;  // cannot happen: lane k is right after round k
    bool changed = false;
    // every lane looks at the exits of the round before, as the wave does
    for (int i = 0; i < lanes; i++) c.prev[i] = c.exitb[i];
    for (int i = 1; i < lanes; i++) {
      if (c.prev[i - 1] == c.start[i]) continue;
      changed = true;
      c.start[i] = c.prev[i - 1];
      HufLaneExit r =
          huf_lane_scan(c.huf, s.src, c.start[i], huf_lane_top(s.T, S, i + 1));
      c.exitb[i] = r.b;
      c.count[i] = r.count;
    }
    if (!changed) break;
  }
  if (rounds > c.rounds) c.rounds = rounds;
  int64_t total = 0;
  for (int i = 0; i < lanes; i++) total += c.count[i];
  if (total != s.outLen || c.exitb[lanes - 1] != 0) return false;
  int64_t off = 0;
  for (int i = 0; i < lanes; i++) {
    huf_lane_write(c.huf, s.src, c.start[i], c.count[i], dst + s.outStart + off);
    off += c.count[i];
  }
  return true;
}

// decode the Huffman-only page frame[0 .. n) into dst[0 .. rs). False, with
// nothing written outside dst[0 .. rs), if the classifier rejects it or any
// stream is invalid. A stream is checked before its own slice is written,
// and by huf4_stream's split every slice lies inside dst[0 .. rs).
inline bool huf_par_decode(const uint8_t* frame, int64_t n, uint8_t* dst,
                           int64_t rs, int lanes, HufParCtx& c) {
  c.rounds = 0;
  HufOnly ho;
  if (lanes < 1 || lanes > kHufParMaxLanes) return false;
  if (!huf_only_frame(frame, n, rs, ho)) return false;
  const uint8_t* p = frame + ho.payload;
  int64_t used = read_huf_tree(p, ho.cs, c.huf, c.ws);
  if (used < 0) return false;
  p += used;
  int64_t rem = ho.cs - used;
  HufParStream s[4];
  for (int i = 0; i < ho.nStreams; i++)
    if (!huf_par_stream(p, rem, rs, ho.nStreams, i, s[i])) return false;
  for (int i = 0; i < ho.nStreams; i++)
    if (!huf_par_stream_host(c, s[i], dst, lanes)) return false;
  return true;
}

}  // namespace lszstd
