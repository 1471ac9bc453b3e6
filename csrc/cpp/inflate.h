// DEFLATE (RFC 1951) with gzip (RFC 1952) and zlib (RFC 1950) framing,
// written from the three format descriptions; no zlib is linked. Parquet
// codec 2 (GZIP) pages are read through inflate_page (compress.h); the GPU
// kernel (csrc/hip/gzip.hip) calls the same bit reader, block header
// parser, table builder, symbol step and framing parsers on every lane and
// does the byte movement itself.
//
// A DEFLATE stream is a run of blocks, each with a 3-bit header (BFINAL,
// BTYPE) read LSB-first:
//   stored   byte-aligned LEN, NLEN (= ~LEN), LEN raw bytes
//   fixed    literal/length and distance codes given by the format
//   dynamic  HLIT, HDIST, HCLEN, a code-length code of up to 19 symbols,
//            then HLIT + HDIST code lengths written with it (symbols
//            16/17/18 repeat; a repeat may run from the literal/length
//            lengths into the distance lengths)
// Symbols of a Huffman block: 0..255 a literal, 256 the end of the block,
// 257..285 a match length (base + extra bits) followed by a distance code
// 0..29 (base + extra bits, 1..32768 back from the output).
//
// Decode tables have two levels with zlib's root sizes (9 bits for
// literal/length, 6 for distance), which bounds them at 852 + 592 entries
// of 4 bytes for any valid set of code lengths; the builder checks the
// bound all the same.
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

// Lanes that split a table fill meet here before anyone reads the table:
// the kernel defines it as its workgroup barrier before it includes this
// file; on the host it is nothing.
#ifndef LSINFL_SYNC
#define LSINFL_SYNC() ((void)0)
#endif

namespace lsinfl {

static const int kLitRoot = 9, kDistRoot = 6, kCodesRoot = 7;
static const int kLitCap = 852, kDistCap = 592;
static const int kMaxLit = 286, kMaxDist = 30;

// table entry: bits 0..7 the bits to consume at this level, 8..15 the op,
// 16..31 a value (literal byte, base length, base distance, sub-table start)
static const uint32_t OP_LIT = 0;      // value is the byte
static const uint32_t OP_BASE = 16;    // | extra bits (0..13), value is the base
static const uint32_t OP_END = 32;     // end of block
static const uint32_t OP_BAD = 64;     // no such code / symbol not allowed
static const uint32_t OP_LINK = 128;   // | index bits of the sub-table

struct Tables {
  uint32_t lit[kLitCap];
  uint32_t dist[kDistCap];
};

// workspace of the dynamic header and the table builder
struct Work {
  uint16_t count[16];   // codes of each length still to be placed
  uint16_t offs[16];
  uint16_t sorted[288];  // symbols in canonical order
  uint8_t lens[320 + 19];  // HLIT + HDIST lengths; the code-length code at 320
};

// -- bit reader: LSB-first, 64-bit buffer; `cnt` counts bits that really
// come from the source, and taking more than that sets `bad` (sticky)
struct Bits {
  const uint8_t* src;
  int64_t n, pos;  // pos: next byte to load
  uint64_t buf;
  int cnt;
  bool bad;
};

LSL4_HD inline void bits_init(Bits& b, const uint8_t* src, int64_t n, int64_t pos) {
  b.src = src;
  b.n = n;
  b.pos = pos;
  b.buf = 0;
  b.cnt = 0;
  b.bad = false;
}

// at least 56 bits afterwards unless the source ends first. The wide load
// may put real stream bits above `cnt`; the next refill writes the same
// bits there again.
LSL4_HD inline void refill(Bits& b) {
  if (b.n - b.pos >= 8) {
    uint64_t w;
    __builtin_memcpy(&w, b.src + b.pos, 8);
    b.buf |= w << b.cnt;
    b.pos += (63 - b.cnt) >> 3;
    b.cnt |= 56;
  } else {
    while (b.cnt <= 56 && b.pos < b.n) {
      b.buf |= (uint64_t)b.src[b.pos++] << b.cnt;
      b.cnt += 8;
    }
  }
}

LSL4_HD inline uint32_t peek(const Bits& b, int k) {
  return (uint32_t)(b.buf & ((1ull << k) - 1));
}

LSL4_HD inline void consume(Bits& b, int k) {
  if (k > b.cnt) {
    b.bad = true;
    k = b.cnt;
  }
  b.buf >>= k;
  b.cnt -= k;
}

LSL4_HD inline uint32_t take(Bits& b, int k) {
  uint32_t v = peek(b, k);
  consume(b, k);
  return v;
}

// drop the rest of the current byte and hand whole unread bytes back:
// returns the byte position the stream continues at, the buffer is empty
LSL4_HD inline int64_t byte_align(Bits& b) {
  consume(b, b.cnt & 7);
  b.pos -= b.cnt >> 3;
  b.buf = 0;
  b.cnt = 0;
  return b.pos;
}

// -- code tables -------------------------------------------------------- //

enum { T_CODES = 0, T_LENS = 1, T_DISTS = 2 };

LSL4_HD inline uint32_t sym_entry(int type, uint32_t sym) {
  if (type == T_CODES) return (sym << 16) | (OP_LIT << 8);
  if (type == T_LENS) {
    if (sym < 256) return (sym << 16) | (OP_LIT << 8);
    if (sym == 256) return OP_END << 8;
    if (sym >= 286) return OP_BAD << 8;
    if (sym == 285) return (258u << 16) | (OP_BASE << 8);
    if (sym < 265) return ((sym - 254) << 16) | (OP_BASE << 8);
    uint32_t e = (sym - 261) >> 2;
    uint32_t base = 3 + ((4 + ((sym - 261) & 3)) << e);
    return (base << 16) | ((OP_BASE | e) << 8);
  }
  if (sym >= 30) return OP_BAD << 8;
  if (sym < 4) return ((sym + 1) << 16) | (OP_BASE << 8);
  uint32_t e = (sym >> 1) - 1;
  uint32_t base = 1 + ((2 + (sym & 1)) << e);
  return (base << 16) | ((OP_BASE | e) << 8);
}

LSL4_HD inline uint32_t bit_reverse(uint32_t v, int n) {
  // n <= 16: swap neighbours, pairs, nibbles, bytes of the 16-bit word
  uint32_t r = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
  r = ((r & 0x3333u) << 2) | ((r >> 2) & 0x3333u);
  r = ((r & 0x0F0Fu) << 4) | ((r >> 4) & 0x0F0Fu);
  r = ((r & 0x00FFu) << 8) | ((r >> 8) & 0x00FFu);
  return r >> (16 - n);
}

// Canonical Huffman decode table of lens[0..n) into table[0..cap). Lane
// `lane` of `nl` writes its share of every replicated entry; the decisions
// are the same on every lane (the host runs lane 0 of 1). False for an
// over-subscribed code, for an incomplete one other than a distance code
// of one 1-bit code or of no code at all, and for a table past cap.
LSL4_HD inline bool build_table(int type, const uint8_t* lens, int n,
                                uint32_t* table, int cap, int root, Work& w,
                                int lane, int nl) {
  LSINFL_SYNC();
  for (int i = 0; i < 16; i++) w.count[i] = 0;
  for (int s = 0; s < n; s++) {
    if (lens[s] > 15) return false;
    w.count[lens[s]]++;
  }
  int max = 15;
  while (max >= 1 && w.count[max] == 0) max--;
  const int rsize = 1 << root;
  if (rsize > cap) return false;
  if (max == 0) {  // no code: every lookup is refused
    if (type != T_DISTS) return false;
    for (int j = lane; j < rsize; j += nl) table[j] = (OP_BAD << 8) | 1;
    LSINFL_SYNC();
    return true;
  }
  int left = 1;
  for (int len = 1; len <= 15; len++) {
    left <<= 1;
    left -= (int)w.count[len];
    if (left < 0) return false;  // over-subscribed
  }
  if (left > 0 && !(type == T_DISTS && max == 1)) return false;  // incomplete
  int o = 0;
  for (int len = 1; len <= 15; len++) {
    w.offs[len] = (uint16_t)o;
    o += w.count[len];
  }
  const int ncodes = o;
  for (int s = 0; s < n; s++)
    if (lens[s]) w.sorted[w.offs[lens[s]]++] = (uint16_t)s;

  if (left > 0) {  // the one code is "0"; "1" is refused
    uint32_t e = sym_entry(type, w.sorted[0]) | 1;
    for (int j = lane; j < rsize; j += nl)
      table[j] = (j & 1) ? ((OP_BAD << 8) | 1) : e;
    LSINFL_SYNC();
    return true;
  }

  uint32_t code = 0;
  int curlen = lens[w.sorted[0]];
  int used = rsize;        // entries taken so far
  int sub = 0, curr = 0;   // the open sub-table: start and index bits
  int64_t low = -1;        // and its root prefix
  const uint32_t rmask = (uint32_t)rsize - 1;
  for (int k = 0; k < ncodes; k++) {
    uint32_t sym = w.sorted[k];
    int len = lens[sym];
    code <<= (len - curlen);
    curlen = len;
    uint32_t rev = bit_reverse(code, len);
    code++;
    uint32_t e = sym_entry(type, sym);
    if (len <= root) {
      e |= (uint32_t)len;
      for (int j = (int)rev + (lane << len); j < rsize; j += nl << len)
        table[j] = e;
    } else {
      if ((int64_t)(rev & rmask) != low) {
        // size the sub-table so that the codes that follow fill it
        curr = len - root;
        int l = 1 << curr;
        while (curr + root < max) {
          l -= (int)w.count[curr + root];
          if (l <= 0) break;
          curr++;
          l <<= 1;
        }
        sub = used;
        used += 1 << curr;
        if (used > cap) return false;
        low = rev & rmask;
        table[low] = ((uint32_t)sub << 16) | ((OP_LINK | (uint32_t)curr) << 8) |
                     (uint32_t)root;
      }
      int sl = len - root;
      e |= (uint32_t)sl;
      for (int j = (int)(rev >> root) + (lane << sl); j < (1 << curr); j += nl << sl)
        table[sub + j] = e;
    }
    w.count[len]--;
  }
  LSINFL_SYNC();
  return true;
}

// one code from `table`; the bits are consumed. OP_BAD for a refused code.
LSL4_HD inline uint32_t decode_entry(Bits& b, const uint32_t* table, int root) {
  uint32_t e = table[peek(b, root)];
  if ((e >> 8) & OP_LINK) {
    consume(b, root);
    int sb = (int)((e >> 8) & 15);
    e = table[(e >> 16) + peek(b, sb)];
    if ((e >> 8) & OP_LINK) return OP_BAD << 8;
  }
  consume(b, (int)(e & 255));
  return e;
}

// -- blocks ------------------------------------------------------------- //

enum { BLK_STORED = 0, BLK_FIXED = 1, BLK_DYNAMIC = 2 };

struct Block {
  int kind;
  bool last;
  int64_t stored_pos;   // stored: the raw bytes in src
  uint32_t stored_len;
};

// The 3 header bits, and LEN/NLEN of a stored block: its bytes are checked
// to lie inside the source and the reader continues behind them.
LSL4_HD inline bool parse_block_header(Bits& b, Block& blk) {
  refill(b);
  blk.last = take(b, 1) != 0;
  blk.kind = (int)take(b, 2);
  blk.stored_pos = 0;
  blk.stored_len = 0;
  if (b.bad || blk.kind == 3) return false;
  if (blk.kind != BLK_STORED) return true;
  int64_t p = byte_align(b);
  if (b.n - p < 4) return false;
  uint32_t len = (uint32_t)b.src[p] | ((uint32_t)b.src[p + 1] << 8);
  uint32_t nlen = (uint32_t)b.src[p + 2] | ((uint32_t)b.src[p + 3] << 8);
  if ((len ^ nlen) != 0xFFFFu) return false;
  p += 4;
  if ((int64_t)len > b.n - p) return false;
  blk.stored_pos = p;
  blk.stored_len = len;
  b.pos = p + len;
  return true;
}

LSL4_HD inline bool build_fixed(Tables& t, Work& w, int lane, int nl) {
  for (int s = 0; s < 288; s++)
    w.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
  for (int s = 0; s < 32; s++) w.lens[288 + s] = 5;
  return build_table(T_LENS, w.lens, 288, t.lit, kLitCap, kLitRoot, w, lane, nl) &&
         build_table(T_DISTS, w.lens + 288, 32, t.dist, kDistCap, kDistRoot, w,
                     lane, nl);
}

// position i of the code-length code's lengths in the header
LSL4_HD inline int clen_order(int i) {
  // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, 5 bits each
  const uint64_t lo = 16ull | (17ull << 5) | (18ull << 10) | (0ull << 15) |
                      (8ull << 20) | (7ull << 25) | (9ull << 30) | (6ull << 35) |
                      (10ull << 40) | (5ull << 45) | (11ull << 50) | (4ull << 55);
  const uint64_t hi = 12ull | (3ull << 5) | (13ull << 10) | (2ull << 15) |
                      (14ull << 20) | (1ull << 25) | (15ull << 30);
  return i < 12 ? (int)((lo >> (5 * i)) & 31) : (int)((hi >> (5 * (i - 12))) & 31);
}

// header of a dynamic block: both tables built, or false
LSL4_HD inline bool build_dynamic(Bits& b, Tables& t, Work& w, int lane, int nl) {
  refill(b);
  int hlit = (int)take(b, 5) + 257;
  int hdist = (int)take(b, 5) + 1;
  int hclen = (int)take(b, 4) + 4;
  if (b.bad || hlit > kMaxLit || hdist > kMaxDist) return false;
  uint8_t* cl = w.lens + 320;
  for (int i = 0; i < 19; i++) cl[i] = 0;
  for (int i = 0; i < hclen; i++) {
    if ((i & 7) == 0) refill(b);
    cl[clen_order(i)] = (uint8_t)take(b, 3);
  }
  if (b.bad) return false;
  if (!build_table(T_CODES, cl, 19, t.lit, kLitCap, kCodesRoot, w, lane, nl))
    return false;
  const int total = hlit + hdist;
  int i = 0;
  while (i < total) {
    refill(b);
    uint32_t e = decode_entry(b, t.lit, kCodesRoot);
    if (((e >> 8) & 255) != OP_LIT) return false;
    uint32_t sym = e >> 16;
    if (sym < 16) {
      w.lens[i++] = (uint8_t)sym;
    } else {
      uint8_t prev = 0;
      int rep;
      if (sym == 16) {
        if (i == 0) return false;
        prev = w.lens[i - 1];
        rep = 3 + (int)take(b, 2);
      } else if (sym == 17) {
        rep = 3 + (int)take(b, 3);
      } else {
        rep = 11 + (int)take(b, 7);
      }
      if (i + rep > total) return false;
      while (rep--) w.lens[i++] = prev;
    }
    if (b.bad) return false;
  }
  if (w.lens[256] == 0) return false;  // no end-of-block code
  return build_table(T_LENS, w.lens, hlit, t.lit, kLitCap, kLitRoot, w, lane, nl) &&
         build_table(T_DISTS, w.lens + hlit, hdist, t.dist, kDistCap, kDistRoot,
                     w, lane, nl);
}

enum { SYM_LIT = 0, SYM_END = 1, SYM_MATCH = 2, SYM_BAD = 3 };

struct Sym {
  uint32_t lit;   // SYM_LIT
  uint32_t len;   // SYM_MATCH: 3..258
  uint32_t dist;  // SYM_MATCH: 1..32768
};

// One symbol of a Huffman block: a literal, the end of the block, or a
// match with length and distance resolved (at most 15+5+15+13 bits, one
// refill). SYM_BAD for a refused code and for bits past the source.
LSL4_HD inline int parse_symbol(Bits& b, const Tables& t, Sym& s) {
  refill(b);
  uint32_t e = decode_entry(b, t.lit, kLitRoot);
  uint32_t op = (e >> 8) & 255;
  if (op == OP_LIT) {
    s.lit = e >> 16;
    return b.bad ? SYM_BAD : SYM_LIT;
  }
  if (op == OP_END) return b.bad ? SYM_BAD : SYM_END;
  if (!(op & OP_BASE) || (op & OP_BAD)) return SYM_BAD;
  s.len = (e >> 16) + take(b, (int)(op & 15));
  e = decode_entry(b, t.dist, kDistRoot);
  op = (e >> 8) & 255;
  if (!(op & OP_BASE) || (op & OP_BAD)) return SYM_BAD;
  s.dist = (e >> 16) + take(b, (int)(op & 15));
  return b.bad ? SYM_BAD : SYM_MATCH;
}

// -- framing ------------------------------------------------------------ //

LSL4_HD inline bool is_gzip(const uint8_t* src, int64_t n) {
  return n >= 2 && src[0] == 0x1f && src[1] == 0x8b;
}

// gzip member header at src[pos]: pos moves to the DEFLATE stream
LSL4_HD inline bool gzip_header(const uint8_t* src, int64_t n, int64_t& pos) {
  if (pos < 0 || n - pos < 10) return false;
  if (src[pos] != 0x1f || src[pos + 1] != 0x8b || src[pos + 2] != 8) return false;
  const uint8_t flg = src[pos + 3];
  if (flg & 0xE0) return false;  // reserved bits
  int64_t p = pos + 10;
  if (flg & 4) {  // FEXTRA
    if (n - p < 2) return false;
    int64_t xlen = (int64_t)src[p] | ((int64_t)src[p + 1] << 8);
    p += 2;
    if (xlen > n - p) return false;
    p += xlen;
  }
  for (int f = 8; f <= 16; f <<= 1) {  // FNAME, FCOMMENT: zero-terminated
    if (!(flg & f)) continue;
    while (p < n && src[p]) p++;
    if (p >= n) return false;
    p++;
  }
  if (flg & 2) {  // FHCRC
    if (n - p < 2) return false;
    p += 2;
  }
  pos = p;
  return true;
}

// zlib stream header at src[pos] (RFC 1950): no preset dictionary
LSL4_HD inline bool zlib_header(const uint8_t* src, int64_t n, int64_t& pos) {
  if (pos < 0 || n - pos < 2) return false;
  const uint32_t cmf = src[pos], flg = src[pos + 1];
  if ((cmf & 15) != 8 || (cmf >> 4) > 7) return false;
  if (((cmf << 8) | flg) % 31) return false;
  if (flg & 0x20) return false;
  pos += 2;
  return true;
}

LSL4_HD inline uint32_t le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) |
         ((uint32_t)p[3] << 24);
}

LSL4_HD inline uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) |
         ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

// -- host decoder ------------------------------------------------------- //

// One DEFLATE stream from src[pos] into dst[0..cap): `pos` ends up behind
// its last byte, `produced` is the output length. Distances count back
// from dst, the start of this stream's output.
LSL4_HD inline bool inflate_stream(uint8_t* dst, int64_t cap, const uint8_t* src,
                                   int64_t n, int64_t& pos, int64_t& produced,
                                   Tables& t, Work& w) {
  Bits b;
  bits_init(b, src, n, pos);
  int64_t d = 0;
  bool have_fixed = false;
  for (;;) {
    Block blk;
    if (!parse_block_header(b, blk)) return false;
    if (blk.kind == BLK_STORED) {
      if ((int64_t)blk.stored_len > cap - d) return false;
      for (uint32_t i = 0; i < blk.stored_len; i++) dst[d + i] = src[blk.stored_pos + i];
      d += blk.stored_len;
    } else {
      if (blk.kind == BLK_FIXED) {
        if (!have_fixed && !build_fixed(t, w, 0, 1)) return false;
        have_fixed = true;
      } else {
        have_fixed = false;
        if (!build_dynamic(b, t, w, 0, 1)) return false;
      }
      for (;;) {
        Sym s;
        int k = parse_symbol(b, t, s);
        if (k == SYM_LIT) {
          if (d >= cap) return false;
          dst[d++] = (uint8_t)s.lit;
        } else if (k == SYM_MATCH) {
          if ((int64_t)s.dist > d) return false;
          if ((int64_t)s.len > cap - d) return false;
          const uint8_t* from = dst + d - s.dist;
          for (uint32_t i = 0; i < s.len; i++) dst[d + i] = from[i];  // may overlap
          d += s.len;
        } else if (k == SYM_END) {
          break;
        } else {
          return false;
        }
      }
    }
    if (blk.last) break;
  }
  pos = byte_align(b);
  if (b.bad) return false;
  produced = d;
  return true;
}

}  // namespace lsinfl

#if !defined(__HIP_DEVICE_COMPILE__)
namespace lsinfl {

inline uint32_t crc32(const uint8_t* p, int64_t n) {
  struct Table {
    uint32_t t[256];
    Table() {
      for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1)));
        t[i] = c;
      }
    }
  };
  static const Table tab;
  uint32_t c = 0xFFFFFFFFu;
  for (int64_t i = 0; i < n; i++) c = tab.t[(c ^ p[i]) & 255] ^ (c >> 8);
  return ~c;
}

inline uint32_t adler32(const uint8_t* p, int64_t n) {
  uint32_t a = 1, b = 0;
  while (n > 0) {
    int64_t k = n < 5552 ? n : 5552;  // the sums cannot wrap in 5552 steps
    for (int64_t i = 0; i < k; i++) {
      a += p[i];
      b += a;
    }
    a %= 65521;
    b %= 65521;
    p += k;
    n -= k;
  }
  return (b << 16) | a;
}

// A bare DEFLATE stream of exactly src_n bytes into exactly dst_n bytes.
inline bool inflate_raw(uint8_t* dst, int64_t dst_n, const uint8_t* src,
                        int64_t src_n) {
  if (dst_n < 0 || src_n < 0) return false;
  Tables t;
  Work w;
  int64_t pos = 0, got = 0;
  return inflate_stream(dst, dst_n, src, src_n, pos, got, t, w) &&
         pos == src_n && got == dst_n;
}

// A parquet GZIP page: one or more gzip members back to back (CRC32 and
// ISIZE of each verified), or one zlib stream (Adler-32 verified), which
// some writers put under the codec. False on any damage, on bytes behind
// the last member and when the output is not exactly dst_n bytes. Reads
// only [src, src + src_n), writes only [dst, dst + dst_n).
inline bool inflate_page(uint8_t* dst, int64_t dst_n, const uint8_t* src,
                         int64_t src_n) {
  if (dst_n < 0 || src_n < 2) return false;
  Tables t;
  Work w;
  int64_t pos = 0, d = 0, got = 0;
  if (!is_gzip(src, src_n)) {
    if (!zlib_header(src, src_n, pos)) return false;
    if (!inflate_stream(dst, dst_n, src, src_n, pos, got, t, w)) return false;
    if (src_n - pos != 4 || got != dst_n) return false;
    return be32(src + pos) == adler32(dst, got);
  }
  while (pos < src_n) {
    if (!gzip_header(src, src_n, pos)) return false;
    if (!inflate_stream(dst + d, dst_n - d, src, src_n, pos, got, t, w)) return false;
    if (src_n - pos < 8) return false;
    if (le32(src + pos) != crc32(dst + d, got)) return false;
    if (le32(src + pos + 4) != (uint32_t)got) return false;
    pos += 8;
    d += got;
  }
  return d == dst_n;
}

}  // namespace lsinfl
#endif
