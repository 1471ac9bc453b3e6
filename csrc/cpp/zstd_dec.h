// From-scratch zstd *decoder* (RFC 8878 subset: everything libzstd's
// compressor emits — raw/RLE/compressed blocks, huffman literals with
// direct or FSE-compressed weights, 1/4-stream literals, predefined /
// RLE / FSE / repeat sequence tables, repeat offsets, multi-block
// frames; no dictionaries, no checksum verification).
//
// Shared with the GPU kernel (csrc/hip/zstd.hip), which includes this
// file: the bit readers, the FSE / huffman table builders and every
// function that knows the layout of a frame (frame, block and literals
// headers, huffman tree description, 4-stream layout, sequence count,
// sequence tables, one sequence). Those are LSZ_HD, pure functions of the
// input bytes and small lane-uniform state: they move no output bytes and
// never synchronise. Per side: the byte movement and its fencing — the
// host drivers at the end of this file use memcpy, the device drivers use
// wave-cooperative copies. No STL containers in the decode path,
// fixed-size scratch tables, plain C-style code. The host build is
// differential-tested against libzstd on real parquet pages
// (tests/test_zstd_dec.py), so the device's parse and bounds checks carry
// that coverage too.
//
// This replaces host-side libzstd in the GPU scan path so page
// decompression scales with the GPU instead of the (cgroup-capped) CPU
// quota — see SURVEY.md §7.2 (reference decompresses on tokio threads,
// arrow-rs parquet; we aim the same bytes at the MI355X).

#pragma once

#include <cstdint>
#include <cstring>

#ifndef LSZ_HD
#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#define LSZ_HD __host__ __device__
#define LSZ_COLD __host__ __device__ __attribute__((noinline))
#else
#define LSZ_HD
#define LSZ_COLD
#endif
#endif

namespace lszstd {

static const uint32_t kMagic = 0xFD2FB528u;

LSZ_HD inline int highbit32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return 31 - __clz(v);
#elif defined(__GNUC__)
  return 31 - __builtin_clz(v);
#else
  int r = 0;
  while (v >>= 1) r++;
  return r;
#endif
}

// ---------------------------------------------------------------------- //
// backward bitstream: bits were appended LSB-first; the reader starts at
// the sentinel (highest set bit of the last byte) and reads downward.
// Reads past the start return zero bits and set `overflow`.
// ---------------------------------------------------------------------- //

struct BitBwd {
  const uint8_t* buf;
  int64_t bitpos;    // bits remaining below the cursor
  uint64_t cont;     // register window: stream bits [contEnd-64, contEnd)
  int64_t contEnd;   // byte-aligned top of the window (bit index)
  bool overflow;

  LSZ_HD void refill() {
    // place an 8-byte window ending at the cursor byte; never reads past
    // the buffer end (bits exist => bytes do) and zero-pads small bufs
    int64_t byteHi = (bitpos + 7) >> 3;
    if (byteHi >= 8) {
      memcpy(&cont, buf + byteHi - 8, 8);
      contEnd = byteHi * 8;
    } else {
      uint64_t w = 0;
      for (int64_t i = 0; i < byteHi; i++) w |= (uint64_t)buf[i] << (8 * i);
      contEnd = 64;          // treat bits [0,64); bits >= byteHi*8 unused
      cont = w;
    }
  }

  LSZ_HD bool init(const uint8_t* p, int64_t n) {
    buf = p;
    overflow = false;
    cont = 0;
    contEnd = 0;
    if (n <= 0) { bitpos = 0; overflow = true; return false; }
    uint8_t last = p[n - 1];
    if (last == 0) { bitpos = 0; overflow = true; return false; }
    bitpos = (n - 1) * 8 + highbit32(last);  // sentinel bit excluded
    refill();
    return true;
  }

  // read n bits [bitpos-n, bitpos); zero-padded when under-running
  LSZ_HD uint32_t read(int n) {
    if (n == 0) return 0;
    if (bitpos - n < contEnd - 64) refill();
    bitpos -= n;
    uint64_t mask = (n >= 32) ? 0xFFFFFFFFull : ((1ull << n) - 1);
    int64_t shift = bitpos - (contEnd - 64);
    if (bitpos < 0) overflow = true;
    if (shift >= 0) return (uint32_t)((cont >> shift) & mask);
    // under-run: stream bits below 0 read as zeros
    if (shift <= -64) return 0;
    return (uint32_t)((cont << (-shift)) & mask);
  }

  LSZ_HD bool done() const { return bitpos <= 0; }
};

// forward bitstream (FSE table descriptions), LSB-first
struct BitFwd {
  const uint8_t* buf;
  int64_t n;
  int64_t bitpos = 0;

  LSZ_HD uint32_t read(int nb) {
    uint32_t out = 0;
    for (int i = 0; i < nb; i++) {
      int64_t b = bitpos + i;
      if ((b >> 3) < n) out |= (uint32_t)((buf[b >> 3] >> (b & 7)) & 1) << i;
    }
    bitpos += nb;
    return out;
  }
  LSZ_HD uint32_t peek(int nb) const {
    uint32_t out = 0;
    for (int i = 0; i < nb; i++) {
      int64_t b = bitpos + i;
      if ((b >> 3) < n) out |= (uint32_t)((buf[b >> 3] >> (b & 7)) & 1) << i;
    }
    return out;
  }
  LSZ_HD int64_t bytes_consumed() const { return (bitpos + 7) >> 3; }
};

// ---------------------------------------------------------------------- //
// FSE
// ---------------------------------------------------------------------- //

static const int kHufMaxBits = 11;  // zstd huffman log limit
static const int kMaxTableLog = 9;          // zstd: OF 8, ML 9, LL 9, weights 6
static const int kMaxSymbols = 256;

struct FseEntry {
  uint8_t symbol;
  uint8_t nbBits;
  uint16_t newState;  // baseline; nextState = newState + read(nbBits)
};

struct FseTable {  // no default initializers: instances live in LDS
  FseEntry e[1 << kMaxTableLog];
  int tableLog;
  bool rle;          // degenerate: single symbol, no bits
  uint8_t rleSym;
};

// table-build workspace. The host keeps one in Ctx, the device one in LDS
// for lane 0 (dynamically-indexed locals would otherwise force a multi-KB
// private segment per lane that craters wave residency).
struct BuildWs {
  FseTable wt;                         // huffman-weight FSE table
  int16_t counts[kMaxSymbols];         // normalized counts
  uint16_t symNext[kMaxSymbols];
  uint8_t symTab[1 << kMaxTableLog];
  uint8_t weights[kMaxSymbols];        // huffman weights
  uint32_t rankCount[16], rankStart[16];  // huf_build: symbols / cells per weight
};

// read normalized counts (RFC 8878 4.1.1) from a forward bitstream.
// returns max symbol (inclusive) or -1 on error.
LSZ_HD inline int fse_read_ncount_br(BitFwd& br, int16_t* counts,
                                     int maxSymLimit, int& tableLog) {
  tableLog = (int)br.read(4) + 5;
  if (tableLog > kMaxTableLog) return -1;
  int32_t remaining = (1 << tableLog) + 1;
  int sym = 0;
  bool prev0 = false;
  for (int i = 0; i <= maxSymLimit; i++) counts[i] = 0;
  while (remaining > 1 && sym <= maxSymLimit) {
    if (prev0) {
      // runs of zero-probability symbols: 2-bit repeat counts
      int rpt = (int)br.read(2);
      sym += rpt;
      while (rpt == 3) {
        rpt = (int)br.read(2);
        sym += rpt;
      }
      prev0 = false;
      if (sym > maxSymLimit) return -1;
      continue;
    }
    int nbBits = highbit32((uint32_t)remaining) + 1;
    uint32_t val = br.peek(nbBits);
    uint32_t lowMask = (1u << (nbBits - 1)) - 1;
    uint32_t threshold = (uint32_t)((1 << nbBits) - 1 - remaining);
    if ((val & lowMask) < threshold) {
      br.read(nbBits - 1);
      val &= lowMask;
    } else {
      br.read(nbBits);
      val &= (1u << nbBits) - 1;
      if (val >= lowMask + 1) val -= threshold;  // fold the high range
    }
    int32_t count = (int32_t)val - 1;  // -1 means "less than one"
    if (count == -1) {
      counts[sym] = -1;
      remaining -= 1;
    } else {
      counts[sym] = (int16_t)count;
      remaining -= count;
      if (count == 0) prev0 = true;
    }
    sym++;
  }
  if (remaining != 1) return -1;
  return sym - 1;
}

struct NCount {
  int maxSym;        // -1 on error
  int tableLog;
  int64_t consumed;  // bytes of the description
};

// the same from src[0..n). Returns by value, so that on the device (where
// this is not inlined) the bit reader lives in this function's frame and
// not in the kernel's private segment.
LSZ_COLD inline NCount fse_read_ncount(const uint8_t* src, int64_t n,
                                       int16_t* counts, int maxSymLimit) {
  BitFwd br{src, n};
  NCount r;
  r.maxSym = fse_read_ncount_br(br, counts, maxSymLimit, r.tableLog);
  r.consumed = br.bytes_consumed();
  return r;
}

// build a decode table from the normalized counts in ws.counts
// (FSE_buildDTable)
LSZ_COLD inline bool fse_build(FseTable& t, int maxSym, int tableLog,
                               BuildWs& ws) {
  const int16_t* counts = ws.counts;
  uint8_t* symTab = ws.symTab;
  uint16_t* symbolNext = ws.symNext;
  t.tableLog = tableLog;
  t.rle = false;
  int tableSize = 1 << tableLog;
  int highThreshold = tableSize - 1;

  for (int s = 0; s <= maxSym; s++) {
    if (counts[s] == -1) {
      symTab[highThreshold--] = (uint8_t)s;
      symbolNext[s] = 1;
    } else {
      symbolNext[s] = (uint16_t)counts[s];
    }
  }
  // spread symbols
  int step = (tableSize >> 1) + (tableSize >> 3) + 3;
  int mask = tableSize - 1;
  int pos = 0;
  for (int s = 0; s <= maxSym; s++) {
    for (int i = 0; i < counts[s]; i++) {
      symTab[pos] = (uint8_t)s;
      pos = (pos + step) & mask;
      while (pos > highThreshold) pos = (pos + step) & mask;
    }
  }
  if (pos != 0) return false;
  // state transitions
  for (int u = 0; u < tableSize; u++) {
    uint8_t s = symTab[u];
    uint16_t nextState = symbolNext[s]++;
    int nbBits = tableLog - highbit32(nextState);
    t.e[u].symbol = s;
    t.e[u].nbBits = (uint8_t)nbBits;
    t.e[u].newState = (uint16_t)((nextState << nbBits) - tableSize);
  }
  return true;
}

LSZ_HD inline void fse_build_rle(FseTable& t, uint8_t sym) {
  t.rle = true;
  t.rleSym = sym;
  t.tableLog = 0;
  t.e[0].symbol = sym;
  t.e[0].nbBits = 0;
  t.e[0].newState = 0;
}

struct FseState {
  uint32_t state;
  LSZ_HD void init(const FseTable& t, BitBwd& br) {
    state = t.rle ? 0 : br.read(t.tableLog);
  }
  LSZ_HD uint8_t symbol(const FseTable& t) const { return t.e[state].symbol; }
  LSZ_HD void update(const FseTable& t, BitBwd& br) {
    if (t.rle) return;
    const FseEntry& e = t.e[state];
    state = e.newState + br.read(e.nbBits);
  }
};

// generic FSE decompression (used for huffman weights): strict s1/s2
// alternation, stop after overflow emits the final symbol (libzstd
// FSE_decompress_usingDTable tail semantics). dst must not alias ws.wt /
// ws.counts / ws.symTab / ws.symNext; ws.weights is fine.
LSZ_COLD inline int fse_decompress_ws(const uint8_t* src, int64_t n, uint8_t* dst,
                                    int dstCap, BuildWs& ws) {
  FseTable& table = ws.wt;
  NCount nc = fse_read_ncount(src, n, ws.counts, 255);
  if (nc.maxSym < 0) return -1;
  if (!fse_build(table, nc.maxSym, nc.tableLog, ws)) return -1;
  int64_t consumed = nc.consumed;
  BitBwd br;
  if (!br.init(src + consumed, n - consumed)) return -1;
  FseState s1, s2;
  s1.init(table, br);
  s2.init(table, br);
  int out = 0;
  for (;;) {
    if (out >= dstCap) return -1;
    dst[out++] = s1.symbol(table);
    s1.update(table, br);
    if (br.overflow) {
      if (out >= dstCap) return -1;
      dst[out++] = s2.symbol(table);
      break;
    }
    if (out >= dstCap) return -1;
    dst[out++] = s2.symbol(table);
    s2.update(table, br);
    if (br.overflow) {
      if (out >= dstCap) return -1;
      dst[out++] = s1.symbol(table);
      break;
    }
  }
  return out;
}

// ---------------------------------------------------------------------- //
// Huffman literals
// ---------------------------------------------------------------------- //

struct HufEntry {
  uint8_t symbol;
  uint8_t nbBits;
};

struct HufTable {  // no default initializers: instances live in LDS
  HufEntry e[1 << kHufMaxBits];
  int maxBits;
};

// build decode table from weights[0..nsym-1] (HUF_readDTableX1 layout).
// The per-weight counters are indexed by data, so they live in ws (LDS on
// the device) and not in locals: as locals they went to per-lane scratch
// memory, a round trip to global memory for every symbol.
LSZ_COLD inline bool huf_build(HufTable& t, const uint8_t* weights, int nsym,
                               BuildWs& ws) {
  static_assert(kHufMaxBits + 2 <= 16, "rank arrays");
  uint32_t* rankCount = ws.rankCount;
  uint32_t* rankStart = ws.rankStart;
  for (int w = 0; w < kHufMaxBits + 2; w++) rankCount[w] = rankStart[w] = 0;
  uint32_t total = 0;
  for (int s = 0; s < nsym; s++) {
    if (weights[s] > kHufMaxBits) return false;
    rankCount[weights[s]]++;
    if (weights[s]) total += 1u << (weights[s] - 1);
  }
  if (total == 0) return false;
  int maxBits = highbit32(total) + 1;
  if (maxBits > kHufMaxBits) return false;
  // implicit last symbol: fills the gap to the next power of two
  uint32_t rest = (1u << maxBits) - total;
  // rest must be a power of two; its weight:
  if (rest & (rest - 1)) return false;
  int lastWeight = highbit32(rest) + 1;
  t.maxBits = maxBits;

  // table fill: symbols of weight w occupy 2^(w-1) scaled cells; cells
  // are assigned in weight order (low weight = long codes first),
  // symbols of equal weight in symbol order
  {
    uint32_t cur = 0;
    for (int w = 1; w <= maxBits; w++) {
      rankStart[w] = cur;
      uint32_t cells = (rankCount[w] + (w == lastWeight ? 1 : 0))
                       << (w - 1);
      cur += cells;
    }
    if (cur != (1u << maxBits)) return false;
  }
  for (int s = 0; s <= nsym; s++) {
    int w = (s == nsym) ? lastWeight : weights[s];
    if (w == 0) continue;
    uint32_t len = 1u << (w - 1);
    uint32_t start = rankStart[w];
    for (uint32_t i = 0; i < len; i++) {
      t.e[start + i].symbol = (uint8_t)s;
      t.e[start + i].nbBits = (uint8_t)(maxBits + 1 - w);
    }
    rankStart[w] += len;
  }
  return true;
}

// huffman-decode one backward stream into dst[0..outLen)
LSZ_HD inline bool huf_stream(const HufTable& t, const uint8_t* src, int64_t n,
                              uint8_t* dst, int64_t outLen) {
  BitBwd br;
  if (!br.init(src, n)) return outLen == 0;
  uint64_t state = br.read(t.maxBits);  // top maxBits bits
  // reading semantics: state holds the next maxBits bits (MSB-aligned
  // window); after consuming nb bits we shift in nb more from below.
  for (int64_t i = 0; i < outLen; i++) {
    const HufEntry& e = t.e[state];
    dst[i] = e.symbol;
    uint32_t nb = e.nbBits;
    uint32_t more = br.read((int)nb);  // zero-padded past start
    state = ((state << nb) | more) & ((1u << t.maxBits) - 1);
  }
  return true;
}

// ---------------------------------------------------------------------- //
// sequence code tables (RFC 8878 3.1.1.3.2.1)
// ---------------------------------------------------------------------- //

struct CodeExtra {
  uint32_t base;
  uint8_t bits;
};

LSZ_HD inline CodeExtra ll_extra(int code) {
  static const uint32_t base[36] = {
      0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11,   12,   13,   14,   15,
      16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096,
      8192, 16384, 32768, 65536};
  static const uint8_t bits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                   0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3,
                                   4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  return {base[code], bits[code]};
}

LSZ_HD inline CodeExtra ml_extra(int code) {
  static const uint32_t base[53] = {
      3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20,
      21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 37, 39, 41,
      43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387,
      32771, 65539};
  static const uint8_t bits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                   0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                   0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4,
                                   5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
  return {base[code], bits[code]};
}

// predefined distributions (RFC 8878 3.1.1.3.2.2)
LSZ_HD inline void predef_ll(int16_t* c, int& maxSym, int& tlog) {
  static const int16_t d[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2,
                                2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2,
                                2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
  for (int i = 0; i < 36; i++) c[i] = d[i];
  maxSym = 35;
  tlog = 6;
}
LSZ_HD inline void predef_ml(int16_t* c, int& maxSym, int& tlog) {
  static const int16_t d[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1,
                                1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
  for (int i = 0; i < 53; i++) c[i] = d[i];
  maxSym = 52;
  tlog = 6;
}
LSZ_HD inline void predef_of(int16_t* c, int& maxSym, int& tlog) {
  static const int16_t d[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1,
                                1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
  for (int i = 0; i < 29; i++) c[i] = d[i];
  maxSym = 28;
  tlog = 5;
}

// ---------------------------------------------------------------------- //
// format parse functions, shared by the host and device drivers. Each is
// a pure function of the input bytes (and lane-uniform state): no output
// bytes, no synchronisation. Those that build a table write it; the
// device calls only those on a single lane.
// ---------------------------------------------------------------------- //

// frame or skippable-frame header at src[ip] (caller checked ip + 4 <= n).
// Returns the new ip (past a skippable frame, or at the first block
// header) or -1.
LSZ_HD inline int64_t parse_frame_header(const uint8_t* src, int64_t n,
                                         int64_t ip, bool& skippable,
                                         bool& checksum) {
  uint32_t magic;
  memcpy(&magic, src + ip, 4);
  checksum = false;
  skippable = (magic & 0xFFFFFFF0u) == 0x184D2A50u;
  if (skippable) {
    if (ip + 8 > n) return -1;
    uint32_t sz;
    memcpy(&sz, src + ip + 4, 4);
    return ip + 8 + (int64_t)sz;  // 64-bit: a 32-bit sum wraps to ip + 0
  }
  if (magic != kMagic) return -1;
  ip += 4;
  if (ip >= n) return -1;
  uint8_t fhd = src[ip++];
  int fcsFlag = fhd >> 6;
  bool singleSeg = (fhd >> 5) & 1;
  checksum = (fhd >> 2) & 1;
  int dictFlag = fhd & 3;
  if (!singleSeg) {
    if (ip >= n) return -1;
    ip++;  // window descriptor (we size by dstCap)
  }
  ip += (1 << dictFlag) >> 1;  // dictionary id: 0, 1, 2 or 4 bytes
  // content size (informative only): 0/1, 2, 4 or 8 bytes
  ip += fcsFlag == 0 ? (singleSeg ? 1 : 0) : (1 << fcsFlag);
  return ip > n ? -1 : ip;
}

enum { kBlockRaw = 0, kBlockRle = 1, kBlockCompressed = 2 };

struct BlockHdr {
  bool last;
  int type;
  int64_t size;      // raw / RLE: regenerated bytes; compressed: input bytes
  int64_t srcBytes;  // input bytes that follow the 3-byte header
};

// block header at p; fails on the reserved type and when the block's input
// bytes do not fit in rem
LSZ_HD inline bool parse_block_header(const uint8_t* p, int64_t rem,
                                      BlockHdr& h) {
  if (rem < 3) return false;
  uint32_t bh = p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  h.last = bh & 1;
  h.type = (bh >> 1) & 3;
  h.size = bh >> 3;
  h.srcBytes = h.type == kBlockRle ? 1 : h.size;
  return h.type != 3 && 3 + h.srcBytes <= rem;
}

enum { kLitRaw = 0, kLitRle = 1, kLitCompressed = 2, kLitTreeless = 3 };

struct LitHdr {
  int type;
  int sizeFormat;  // the 2-bit header form
  int nStreams;    // huffman streams (compressed / treeless)
  int64_t rs;      // regenerated size
  int64_t cs;      // input bytes after the header (raw: rs, RLE: 1)
  int64_t hdr;     // header length
};

// literals-section header; checks hdr + cs <= n. The caller checks rs
// against its literals buffer.
LSZ_HD inline bool parse_literals_header(const uint8_t* src, int64_t n,
                                         LitHdr& h) {
  if (n < 1) return false;
  h.type = src[0] & 3;
  h.sizeFormat = (src[0] >> 2) & 3;
  h.nStreams = 1;
  if (h.type == kLitRaw || h.type == kLitRle) {
    if ((h.sizeFormat & 1) == 0) {           // 00 or 10: 5-bit size
      h.rs = src[0] >> 3;
      h.hdr = 1;
    } else if (h.sizeFormat == 1) {          // 01: 12-bit
      if (n < 2) return false;
      h.rs = (src[0] >> 4) | ((int64_t)src[1] << 4);
      h.hdr = 2;
    } else {                                 // 11: 20-bit
      if (n < 3) return false;
      h.rs = (src[0] >> 4) | ((int64_t)src[1] << 4) | ((int64_t)src[2] << 12);
      h.hdr = 3;
    }
    h.cs = h.type == kLitRaw ? h.rs : 1;
  } else if (h.sizeFormat <= 1) {  // 1 stream (00) or 4 streams (01), 10-bit
    if (n < 3) return false;
    h.rs = (src[0] >> 4) | ((int64_t)(src[1] & 0x3F) << 4);
    h.cs = (src[1] >> 6) | ((int64_t)src[2] << 2);
    h.hdr = 3;
    h.nStreams = h.sizeFormat == 0 ? 1 : 4;
  } else if (h.sizeFormat == 2) {  // 4 streams, 14-bit
    if (n < 4) return false;
    h.rs = (src[0] >> 4) | ((int64_t)src[1] << 4) | ((int64_t)(src[2] & 3) << 12);
    h.cs = (src[2] >> 2) | ((int64_t)src[3] << 6);
    h.hdr = 4;
    h.nStreams = 4;
  } else {  // 4 streams, 18-bit
    if (n < 5) return false;
    h.rs = (src[0] >> 4) | ((int64_t)src[1] << 4) | ((int64_t)(src[2] & 0x3F) << 12);
    h.cs = (src[2] >> 6) | ((int64_t)src[3] << 2) | ((int64_t)src[4] << 10);
    h.hdr = 5;
    h.nStreams = 4;
  }
  return h.hdr + h.cs <= n;
}

// first byte of a huffman tree description: direct 4-bit weights, or
// FSE-compressed weights
LSZ_HD inline bool huf_desc_direct(uint8_t hb) { return hb >= 128; }

// huffman tree description at p: weights into ws, decode table into t.
// Returns bytes consumed or -1.
LSZ_HD inline int64_t read_huf_tree(const uint8_t* p, int64_t rem,
                                    HufTable& t, BuildWs& ws) {
  if (rem < 1) return -1;
  uint8_t hb = p[0];
  int nw;
  int64_t used;
  if (huf_desc_direct(hb)) {
    nw = hb - 127;
    used = 1 + (nw + 1) / 2;
    if (used > rem) return -1;
    for (int i = 0; i < nw; i++) {
      uint8_t b = p[1 + i / 2];
      ws.weights[i] = (i & 1) ? (b & 0xF) : (b >> 4);
    }
  } else {
    used = 1 + hb;
    if (used > rem) return -1;
    nw = fse_decompress_ws(p + 1, hb, ws.weights, 255, ws);
    if (nw < 0) return -1;
  }
  return huf_build(t, ws.weights, nw, ws) ? used : -1;
}

struct HufStream {
  int64_t start, len;        // input bytes p[start .. start + len)
  int64_t outStart, outLen;  // its slice of the rs regenerated bytes
};

// stream i (0-3) of a 4-stream literals payload: the jump table at p and
// the output split. Whether it fails does not depend on i. (Selects, not
// indexed arrays: the device calls this with i = lane, and an indexed
// local would go to per-lane scratch memory.)
LSZ_HD inline bool huf4_stream(const uint8_t* p, int64_t rem, int64_t rs, int i,
                               HufStream& s) {
  if (rem < 6) return false;
  int64_t s1 = p[0] | ((int64_t)p[1] << 8);
  int64_t s2 = p[2] | ((int64_t)p[3] << 8);
  int64_t s3 = p[4] | ((int64_t)p[5] << 8);
  int64_t s4 = rem - 6 - s1 - s2 - s3;
  int64_t o123 = (rs + 3) / 4;
  int64_t o4 = rs - 3 * o123;
  if (s4 < 0 || o4 < 0) return false;
  s.start = 6 + (i > 0 ? s1 : 0) + (i > 1 ? s2 : 0) + (i > 2 ? s3 : 0);
  s.len = i == 0 ? s1 : i == 1 ? s2 : i == 2 ? s3 : s4;
  s.outStart = i * o123;
  s.outLen = i == 3 ? o4 : o123;
  return true;
}

// number of sequences (1/2/3-byte forms). Returns bytes consumed or -1.
LSZ_HD inline int read_seq_count(const uint8_t* p, int64_t rem, int64_t& nSeq) {
  if (rem < 1) return -1;
  if (p[0] < 128) {
    nSeq = p[0];
    return 1;
  }
  if (p[0] < 255) {
    if (rem < 2) return -1;
    nSeq = ((int64_t)(p[0] - 128) << 8) + p[1];
    return 2;
  }
  if (rem < 3) return -1;
  nSeq = p[1] + ((int64_t)p[2] << 8) + 0x7F00;
  return 3;
}

static const int64_t kHufOnlyMax = 1 << 17;  // largest Huffman-only page

struct HufOnly {
  int nStreams;     // 1 or 4
  int sizeFormat;   // literals header form (10-, 14- or 18-bit sizes)
  int64_t rs;       // regenerated bytes, equals the page's uncompressed size
  int64_t payload;  // src[payload .. payload + cs): tree description, streams
  int64_t cs;
};

// Is src[0..n) a Huffman-only page of `rs` bytes? That is one frame without
// a dictionary id, holding one last compressed block whose literals have
// their own tree and regenerate all `rs` bytes in 1 or 4 streams, followed
// by a sequence count of zero and nothing else. Answered from the header
// bytes; builds no table. Such a page needs no FSE sequence decode, no
// match copy and no window: csrc/cpp/huf_par.h decodes it.
LSZ_HD inline bool huf_only_frame(const uint8_t* src, int64_t n, int64_t rs,
                                  HufOnly& out) {
  if (n < 5 || rs <= 0 || rs > kHufOnlyMax) return false;
  bool skippable, checksum;
  int64_t ip = parse_frame_header(src, n, 0, skippable, checksum);
  if (ip < 0 || skippable || (src[4] & 3) != 0) return false;
  BlockHdr b;
  if (!parse_block_header(src + ip, n - ip, b)) return false;
  if (!b.last || b.type != kBlockCompressed) return false;
  ip += 3;
  if (ip + b.size + (checksum ? 4 : 0) != n) return false;  // one frame only
  LitHdr h;
  if (!parse_literals_header(src + ip, b.size, h)) return false;
  if (h.type != kLitCompressed || h.rs != rs) return false;
  int64_t nSeq;
  int64_t lit = h.hdr + h.cs;
  int used = read_seq_count(src + ip + lit, b.size - lit, nSeq);
  if (used < 0 || nSeq != 0 || lit + used != b.size) return false;
  out.nStreams = h.nStreams;
  out.sizeFormat = h.sizeFormat;
  out.rs = rs;
  out.payload = ip + h.hdr;
  out.cs = h.cs;
  return true;
}

enum { kSeqLL = 0, kSeqOF = 1, kSeqML = 2 };  // table kinds
enum { kModePredef = 0, kModeRle = 1, kModeFse = 2, kModeRepeat = 3 };

// 2-bit mode of table `kind` in the symbol-compression-modes byte
LSZ_HD inline int seq_mode(uint8_t modes, int kind) {
  return (modes >> (6 - 2 * kind)) & 3;
}

// the three sequence decode tables; persist across the blocks of a frame
struct SeqTables {  // no default initializers: instances live in LDS
  FseTable t[3];    // indexed by kind
  bool have[3];
};

// read the table of `kind` per its mode. Returns bytes consumed, -1 err.
// Repeat mode writes nothing. (Inlined on the device too: as a call it
// cost sorted int64 pages about 1 % of their decode time.)
LSZ_HD inline int64_t read_seq_table(SeqTables& st, int kind, int mode,
                                     const uint8_t* src, int64_t n,
                                     BuildWs& ws) {
  const int maxSymLimit = kind == kSeqLL ? 35 : kind == kSeqOF ? 31 : 52;
  FseTable& t = st.t[kind];
  if (mode == kModeRepeat) return st.have[kind] ? 0 : -1;
  int64_t used = 0;
  if (mode == kModeRle) {  // 1 byte symbol
    if (n < 1 || src[0] > maxSymLimit) return -1;
    fse_build_rle(t, src[0]);
    used = 1;
  } else {
    int maxSym, tlog;
    if (mode == kModePredef) {
      if (kind == kSeqLL) predef_ll(ws.counts, maxSym, tlog);
      else if (kind == kSeqOF) predef_of(ws.counts, maxSym, tlog);
      else predef_ml(ws.counts, maxSym, tlog);
    } else {  // FSE table description
      NCount nc = fse_read_ncount(src, n, ws.counts, maxSymLimit);
      if (nc.maxSym < 0) return -1;
      maxSym = nc.maxSym;
      tlog = nc.tableLog;
      used = nc.consumed;
    }
    if (!fse_build(t, maxSym, tlog, ws)) return -1;
  }
  st.have[kind] = true;
  return used;
}

struct SeqStates {
  FseState s[3];  // indexed by kind
  LSZ_HD void init(const SeqTables& st, BitBwd& br) {
    s[kSeqLL].init(st.t[kSeqLL], br);
    s[kSeqOF].init(st.t[kSeqOF], br);
    s[kSeqML].init(st.t[kSeqML], br);
  }
  // between sequences (not after the last one)
  LSZ_HD void update(const SeqTables& st, BitBwd& br) {
    s[kSeqLL].update(st.t[kSeqLL], br);
    s[kSeqML].update(st.t[kSeqML], br);
    s[kSeqOF].update(st.t[kSeqOF], br);
  }
};

struct Seq {
  uint32_t litLen, matchLen, offset;
};

// decode the sequence the states point at: three symbols, their extra
// bits, and the repeat-offset rules (updates rep)
LSZ_HD inline Seq next_sequence(const SeqTables& st, const SeqStates& ss,
                                BitBwd& br, uint32_t* rep) {
  int ofCode = ss.s[kSeqOF].symbol(st.t[kSeqOF]);
  int mlCode = ss.s[kSeqML].symbol(st.t[kSeqML]);
  int llCode = ss.s[kSeqLL].symbol(st.t[kSeqLL]);

  uint32_t ofValue = (ofCode ? (1u << ofCode) : 1u) + br.read(ofCode);
  Seq q;
  CodeExtra mle = ml_extra(mlCode);
  q.matchLen = mle.base + br.read(mle.bits);
  CodeExtra lle = ll_extra(llCode);
  q.litLen = lle.base + br.read(lle.bits);

  if (ofValue > 3) {
    q.offset = ofValue - 3;
    rep[2] = rep[1];
    rep[1] = rep[0];
    rep[0] = q.offset;
  } else {
    uint32_t idx = ofValue - 1 + (q.litLen == 0 ? 1 : 0);
    if (idx == 0) {
      q.offset = rep[0];
    } else {
      uint32_t tmp = (idx == 3) ? rep[0] - 1 : rep[idx];
      if (tmp == 0) tmp = 1;  // corner case per libzstd
      if (idx != 1) rep[2] = rep[1];
      rep[1] = rep[0];
      rep[0] = tmp;
      q.offset = tmp;
    }
  }
  return q;
}

// ---------------------------------------------------------------------- //
// host drivers: parse with the functions above, move bytes with memcpy
// ---------------------------------------------------------------------- //

// decoder context (tables persist across blocks within a frame)
struct Ctx {
  SeqTables seq;
  HufTable huf;
  bool haveHuf = false;
  uint32_t rep[3] = {1, 4, 8};
  BuildWs ws;
  uint8_t litBuf[1 << 17];   // ≤128 KB literals per block
};

// decode literals section; returns bytes consumed from src or -1.
// litLen receives the regenerated length (data in ctx.litBuf).
inline int64_t decode_literals(Ctx& ctx, const uint8_t* src, int64_t n,
                               int64_t& litLen) {
  LitHdr h;
  if (!parse_literals_header(src, n, h)) return -1;
  if (h.rs > (int64_t)sizeof(ctx.litBuf)) return -1;
  litLen = h.rs;
  const uint8_t* p = src + h.hdr;
  if (h.type == kLitRaw) {
    memcpy(ctx.litBuf, p, (size_t)h.rs);
  } else if (h.type == kLitRle) {
    memset(ctx.litBuf, p[0], (size_t)h.rs);
  } else {
    int64_t rem = h.cs;
    if (h.type == kLitCompressed) {  // huffman description present
      int64_t used = read_huf_tree(p, rem, ctx.huf, ctx.ws);
      if (used < 0) return -1;
      ctx.haveHuf = true;
      p += used;
      rem -= used;
    } else if (!ctx.haveHuf) {
      return -1;  // treeless without a previous table
    }
    if (h.nStreams == 1) {
      if (!huf_stream(ctx.huf, p, rem, ctx.litBuf, h.rs)) return -1;
    } else {
      for (int i = 0; i < 4; i++) {
        HufStream s;
        if (!huf4_stream(p, rem, h.rs, i, s)) return -1;
        if (!huf_stream(ctx.huf, p + s.start, s.len, ctx.litBuf + s.outStart,
                        s.outLen))
          return -1;
      }
    }
  }
  return h.hdr + h.cs;
}

// decode one compressed block into dst (history = dst window start..pos)
inline int64_t decode_block(Ctx& ctx, const uint8_t* src, int64_t n,
                            uint8_t* dstBase, int64_t pos, int64_t dstCap) {
  int64_t litLen;
  int64_t used = decode_literals(ctx, src, n, litLen);
  if (used < 0) return -1;
  const uint8_t* p = src + used;
  int64_t rem = n - used;

  int64_t nSeq;
  used = read_seq_count(p, rem, nSeq);
  if (used < 0) return -1;
  p += used; rem -= used;

  if (nSeq == 0) {
    if (pos + litLen > dstCap) return -1;
    memcpy(dstBase + pos, ctx.litBuf, (size_t)litLen);
    return litLen;
  }

  if (rem < 1) return -1;
  uint8_t modes = p[0];
  p += 1; rem -= 1;
  for (int kind = kSeqLL; kind <= kSeqML; kind++) {
    used = read_seq_table(ctx.seq, kind, seq_mode(modes, kind), p, rem, ctx.ws);
    if (used < 0) return -1;
    p += used; rem -= used;
  }

  // execute sequences from the backward bitstream
  BitBwd br;
  if (!br.init(p, rem)) return -1;
  SeqStates ss;
  ss.init(ctx.seq, br);

  int64_t litPos = 0;
  int64_t out = pos;
  for (int64_t s = 0; s < nSeq; s++) {
    Seq q = next_sequence(ctx.seq, ss, br, ctx.rep);

    // copy literals
    if (litPos + q.litLen > litLen || out + q.litLen > dstCap) return -1;
    memcpy(dstBase + out, ctx.litBuf + litPos, q.litLen);
    litPos += q.litLen;
    out += q.litLen;
    // copy match (may overlap)
    if ((int64_t)q.offset > out || out + q.matchLen > dstCap) return -1;
    {
      const uint8_t* from = dstBase + out - q.offset;
      uint8_t* to = dstBase + out;
      if (q.offset >= q.matchLen) {
        memcpy(to, from, q.matchLen);
      } else {
        for (uint32_t i = 0; i < q.matchLen; i++) to[i] = from[i];
      }
      out += q.matchLen;
    }

    if (s + 1 < nSeq) {  // last sequence: no state update
      ss.update(ctx.seq, br);
      if (br.overflow) return -1;
    }
  }
  // trailing literals
  int64_t tail = litLen - litPos;
  if (tail < 0 || out + tail > dstCap) return -1;
  memcpy(dstBase + out, ctx.litBuf + litPos, (size_t)tail);
  out += tail;
  return out - pos;
}

// decode a full zstd frame sequence. Returns decompressed size or -1.
inline int64_t decode(const uint8_t* src, int64_t n, uint8_t* dst,
                      int64_t dstCap, Ctx* ctx) {
  int64_t pos = 0;        // output position
  int64_t ip = 0;
  while (ip + 4 <= n) {
    bool skippable, checksum;
    ip = parse_frame_header(src, n, ip, skippable, checksum);
    if (ip < 0) return -1;
    if (skippable) continue;

    // reset inter-block context per frame
    ctx->seq.have[0] = ctx->seq.have[1] = ctx->seq.have[2] = false;
    ctx->haveHuf = false;
    ctx->rep[0] = 1; ctx->rep[1] = 4; ctx->rep[2] = 8;

    BlockHdr b;
    do {
      if (!parse_block_header(src + ip, n - ip, b)) return -1;
      ip += 3;
      if (b.type == kBlockCompressed) {
        int64_t outb = decode_block(*ctx, src + ip, b.size, dst, pos, dstCap);
        if (outb < 0) return -1;
        pos += outb;
      } else {
        if (pos + b.size > dstCap) return -1;
        if (b.type == kBlockRaw) memcpy(dst + pos, src + ip, (size_t)b.size);
        else memset(dst + pos, src[ip], (size_t)b.size);
        pos += b.size;
      }
      ip += b.srcBytes;
    } while (!b.last);
    if (checksum) ip += 4;
  }
  return pos;
}

}  // namespace lszstd
