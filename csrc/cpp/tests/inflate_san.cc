// Bounds check of the DEFLATE decoder (csrc/cpp/inflate.h) — built with
// -fsanitize=address,undefined by tests/test_gzip.py::test_gzip_sanitizer_clean.
// Input and output sit in exactly-sized heap buffers, so any read or write
// past either end is a sanitizer report.
// - Streams made here (stored blocks, fixed-Huffman blocks with matches up
//   to length 258 and distance 32768) of column-shaped data at 0 B to
//   128 KB, under gzip and zlib framing and as two members, decode back to
//   their input; a page one byte larger or smaller is refused.
// - Recorded streams with dynamic blocks: a zlib level-9 page, a 15-bit
//   code, a distance code of one 1-bit code, a repeat code that runs from
//   the literal/length lengths into the distance lengths.
// - Each small page is truncated at every length, has every byte replaced
//   by four other values and gets trailing garbage: each decode fails or
//   yields exactly the page's size.
// - The table builder run as 64 lanes (the GPU kernel's split of the fill,
//   csrc/hip/gzip.hip) gives the table of the one-lane run.
// The bit reader, header parsers, table builder and symbol step under test
// are the ones the kernel runs; it has no sanitizer of its own.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../inflate.h"

using Bytes = std::vector<uint8_t>;

static long g_runs = 0, g_failed = 0;

static uint32_t g_lcg = 2463534242u;
static uint32_t rnd() {
  g_lcg = g_lcg * 1664525u + 1013904223u;
  return g_lcg >> 8;
}

// recorded streams (zlib's encoder and a bit-by-bit writer made them)
static const uint8_t kDynamicPage[273] = {
    0x1f, 0x8b, 0x08, 0x00, 0x00, 0x00, 0x00, 0x00, 0x02, 0x03, 0x45, 0x92, 0x3b, 0x6e, 0x04, 0x31,
    0x0c, 0x43, 0xaf, 0x64, 0x7d, 0x6d, 0x61, 0xa1, 0xb3, 0xa4, 0xd8, 0x36, 0x40, 0xee, 0xdf, 0x45,
    0x98, 0x25, 0xbd, 0x95, 0x07, 0x03, 0x88, 0x7c, 0x22, 0xf5, 0xfe, 0xfb, 0xfd, 0x59, 0xbd, 0x5e,
    0xef, 0x79, 0xa5, 0xe5, 0x79, 0xb5, 0xfd, 0x79, 0xad, 0xeb, 0x79, 0xbd, 0x25, 0x9f, 0x8f, 0x68,
    0x8d, 0xe7, 0x23, 0xdb, 0x3e, 0x7f, 0x56, 0x7b, 0x61, 0x36, 0x1d, 0xc3, 0x47, 0x30, 0x2d, 0x6b,
    0x71, 0x5e, 0x05, 0x02, 0xe2, 0x0e, 0x05, 0xc9, 0x82, 0x84, 0x54, 0x42, 0x43, 0xa1, 0xaf, 0x63,
    0x94, 0x50, 0xd1, 0x43, 0x0a, 0x53, 0x87, 0x8a, 0xa5, 0x40, 0xc5, 0xe1, 0x31, 0x20, 0x2e, 0x50,
    0xf1, 0x43, 0x94, 0xd0, 0x82, 0x4a, 0xec, 0x84, 0x4a, 0xc2, 0x23, 0x3a, 0xf1, 0x2f, 0x7b, 0x2b,
    0x59, 0x36, 0x66, 0xa5, 0x8f, 0x33, 0x8d, 0x82, 0xc7, 0xe4, 0x01, 0x5f, 0xef, 0x8b, 0x02, 0xba,
    0xd9, 0x27, 0x18, 0x09, 0xb7, 0x98, 0x7d, 0xb0, 0x99, 0x0e, 0x31, 0x49, 0x1c, 0x09, 0xf8, 0xd0,
    0x31, 0x95, 0x84, 0x43, 0x76, 0x22, 0xbd, 0x21, 0xc9, 0x2f, 0x49, 0x91, 0xc4, 0x6e, 0x2a, 0xc1,
    0x68, 0xbf, 0xdd, 0x2c, 0xa2, 0xd8, 0x72, 0x86, 0xb2, 0x18, 0x4a, 0xc0, 0x42, 0xc7, 0x8c, 0x05,
    0xed, 0x45, 0x94, 0x83, 0xd9, 0xe8, 0x12, 0x86, 0x02, 0x8b, 0xe9, 0xc7, 0x6e, 0x3f, 0x97, 0xc4,
    0x92, 0x37, 0xe2, 0x87, 0x99, 0x70, 0x8b, 0x98, 0x3c, 0xd9, 0xcf, 0x71, 0xa2, 0x54, 0xf2, 0x52,
    0x6e, 0x28, 0x0c, 0xca, 0xda, 0x82, 0xf5, 0xf8, 0x21, 0x49, 0x2a, 0x4f, 0x65, 0x27, 0x43, 0x61,
    0x15, 0x53, 0x32, 0xdb, 0x91, 0x43, 0x12, 0x53, 0x5e, 0x8a, 0xef, 0xbc, 0x22, 0xbc, 0xd8, 0xbd,
    0xd9, 0x4f, 0x69, 0xdd, 0x64, 0x49, 0x32, 0x72, 0xff, 0x1b, 0xe8, 0x43, 0x2d, 0x0b, 0x03, 0x00,
    0x00,
};
static const uint8_t kRaw15Bit[343] = {
    0x05, 0xe0, 0x01, 0x96, 0x24, 0x49, 0x92, 0x24, 0x59, 0x7e, 0x40, 0x62, 0x51, 0xf3, 0xc8, 0xea,
    0xd9, 0xfb, 0x1f, 0x77, 0xdf, 0x7f, 0xf7, 0xff, 0xfb, 0xff, 0xd9, 0xf6, 0xef, 0xfb, 0xbb, 0xff,
    0xdf, 0xff, 0xfe, 0x6b, 0xff, 0xdf, 0xfb, 0x7f, 0xff, 0xe7, 0xef, 0xdf, 0x5f, 0xff, 0xbb, 0xef,
    0xf7, 0x7e, 0xff, 0xef, 0xef, 0xff, 0xfe, 0xbf, 0xbb, 0x7f, 0xfb, 0xdf, 0xff, 0xfe, 0xf7, 0xff,
    0xfb, 0xfd, 0x7f, 0xff, 0xbf, 0xff, 0xef, 0xf9, 0x7f, 0xff, 0xbf, 0xf7, 0xdf, 0xfe, 0xbf, 0xff,
    0xf7, 0xfb, 0xbf, 0xfb, 0xff, 0xfd, 0xdf, 0xff, 0xfb, 0xcf, 0xff, 0xfd, 0xef, 0xfe, 0xdf, 0xbe,
    0xff, 0xfb, 0x3f, 0xf7, 0xff, 0xfb, 0xb7, 0xef, 0x3f, 0xbf, 0x7b, 0xff, 0xed, 0xff, 0xfb, 0xbf,
    0xff, 0xfe, 0xbf, 0xfe, 0xf7, 0xff, 0xfd, 0xf7, 0xef, 0x7f, 0xff, 0xfb, 0xf7, 0xef, 0xdf, 0xff,
    0xfe, 0xbf, 0xff, 0xf7, 0xfe, 0xbf, 0xfb, 0xef, 0xff, 0xf7, 0xff, 0xfb, 0xff, 0xfd, 0xdf, 0x5f,
    0xff, 0xef, 0xff, 0xfd, 0xdf, 0xbf, 0xff, 0xdf, 0xd7, 0xff, 0xef, 0xff, 0xfb, 0xdf, 0xdf, 0xff,
    0xef, 0xf7, 0xff, 0xfb, 0xdf, 0xff, 0xef, 0xbf, 0xf7, 0xfb, 0xef, 0xf5, 0xff, 0xfd, 0xdf, 0xff,
    0xfb, 0xeb, 0xff, 0xfb, 0xf5, 0x7f, 0xdf, 0xff, 0xf7, 0xdf, 0xff, 0x6f, 0xf7, 0xff, 0xfb, 0xff,
    0xfe, 0x7f, 0xff, 0xfb, 0xff, 0xf5, 0xff, 0xce, 0xd6, 0xef, 0x7f, 0xff, 0x7b, 0x7f, 0xff, 0xfb,
    0xbf, 0xfe, 0xf7, 0xff, 0xed, 0x7f, 0xf7, 0x7f, 0xef, 0xbf, 0xf7, 0xfb, 0xdf, 0xf6, 0xff, 0xfb,
    0xbf, 0xfd, 0xfb, 0xfb, 0xf5, 0xeb, 0xbf, 0xff, 0xfd, 0xfd, 0x7f, 0xff, 0xfb, 0xfd, 0x7f, 0xff,
    0x77, 0xff, 0xef, 0xf7, 0xef, 0xfd, 0xdf, 0xff, 0xbd, 0xbf, 0xb5, 0xe7, 0xeb, 0x7f, 0xff, 0xf7,
    0xfd, 0x7f, 0xd9, 0xff, 0xfe, 0xfb, 0xbf, 0xf7, 0xbf, 0xff, 0xdf, 0xdf, 0xfe, 0xfc, 0xef, 0xef,
    0xfe, 0xdf, 0xff, 0xfd, 0xdb, 0xd3, 0xff, 0xef, 0xaf, 0xff, 0xdb, 0x7f, 0xfe, 0xcf, 0xbf, 0x7e,
    0xff, 0xdf, 0x7f, 0xff, 0xfb, 0xff, 0xfd, 0xce, 0xff, 0xfb, 0x7f, 0x7f, 0x7f, 0xf7, 0xff, 0xfe,
    0xef, 0xef, 0x7f, 0xfd, 0xff, 0xda, 0xff, 0xfd, 0xbb, 0x6f, 0xff, 0xfb, 0xfd, 0xdd, 0xdf, 0xfb,
    0xfe, 0xef, 0xfe, 0xbe, 0xff, 0xdf, 0xf5, 0x7f, 0x6f, 0xff, 0xdf, 0xff, 0x7e, 0xff, 0xbf, 0xff,
    0xdf, 0xff, 0xf7, 0xff, 0xf3, 0xff, 0x07,
};
static const uint8_t kRawSingleDist[15] = {
    0x0d, 0xe0, 0x81, 0x00, 0x00, 0x00, 0x00, 0x80, 0x20, 0xb0, 0xe6, 0x2f, 0xf1, 0x99, 0x05,
};
static const uint8_t kRawRepeatAcross[19] = {
    0x0d, 0xe3, 0x05, 0x01, 0x00, 0x00, 0x00, 0xc2, 0x30, 0x64, 0xdd, 0xfb, 0x87, 0x40, 0x3e, 0xe9,
    0xbe, 0xfe, 0x37,
};

// decode on exactly-sized copies
static bool decode_exact(const Bytes& page, size_t n, Bytes* out, bool raw = false) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[page.size()]), dst(new uint8_t[n]);
  if (!page.empty()) std::memcpy(in.get(), page.data(), page.size());
  bool ok = raw ? lsinfl::inflate_raw(dst.get(), (int64_t)n, in.get(), (int64_t)page.size())
                : lsinfl::inflate_page(dst.get(), (int64_t)n, in.get(), (int64_t)page.size());
  g_runs++;
  if (!ok) g_failed++;
  if (ok && out) out->assign(dst.get(), dst.get() + n);
  return ok;
}

static bool expect(bool cond, const char* what) {
  if (!cond) std::printf("FAIL: %s\n", what);
  return cond;
}

// -- a small encoder: stored blocks and fixed-Huffman blocks ------------- //

struct BitOut {
  Bytes out;
  uint64_t acc = 0;
  int n = 0;
  void bits(uint32_t v, int k) {  // LSB first
    acc |= (uint64_t)(v & ((1u << k) - 1)) << n;
    n += k;
    while (n >= 8) {
      out.push_back((uint8_t)acc);
      acc >>= 8;
      n -= 8;
    }
  }
  void code(uint32_t c, int len) {  // MSB first
    for (int i = len - 1; i >= 0; i--) bits((c >> i) & 1, 1);
  }
  void align() {
    if (n) bits(0, 8 - n);
  }
};

static void fixed_lit(BitOut& w, uint32_t s) {
  if (s < 144) w.code(0x30 + s, 8);
  else if (s < 256) w.code(0x190 + (s - 144), 9);
  else if (s < 280) w.code(s - 256, 7);
  else w.code(0xC0 + (s - 280), 8);
}

static uint32_t g_max_len = 0, g_max_dist = 0;  // what the encoder reached

static void fixed_match(BitOut& w, uint32_t len, uint32_t dist) {
  if (len > g_max_len) g_max_len = len;
  if (dist > g_max_dist) g_max_dist = dist;
  static const uint16_t lb[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27,
                                  31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
                                  227, 258};
  static const uint8_t le[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2,
                                 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  static const uint16_t db[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129,
                                  193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                                  4097, 6145, 8193, 12289, 16385, 24577};
  int li = 28;
  while (lb[li] > len) li--;
  fixed_lit(w, 257 + li);
  w.bits(len - lb[li], le[li]);
  int di = 29;
  while (db[di] > dist) di--;
  w.code(di, 5);
  w.bits(dist - db[di], di < 4 ? 0 : (di >> 1) - 1);
}

// greedy matcher over a hash of 3-byte prefixes, window 32768 (the full
// format range: distance 32768 and length 258 are both emitted)
static void fixed_block(BitOut& w, const Bytes& d, bool last) {
  w.bits(last ? 1 : 0, 1);
  w.bits(1, 2);
  std::vector<int32_t> head(1 << 16, -1);
  size_t i = 0, n = d.size();
  while (i < n) {
    size_t ml = 0, cand = 0;
    if (i + 3 <= n) {
      uint32_t h = ((d[i] | (d[i + 1] << 8) | ((uint32_t)d[i + 2] << 16)) * 2654435761u) >> 16;
      if (head[h] >= 0 && i - (size_t)head[h] <= 32768) {
        cand = (size_t)head[h];
        while (ml < 258 && i + ml < n && d[cand + ml] == d[i + ml]) ml++;
      }
      head[h] = (int32_t)i;
    }
    if (ml >= 3) {
      fixed_match(w, (uint32_t)ml, (uint32_t)(i - cand));
      i += ml;
    } else {
      fixed_lit(w, d[i++]);
    }
  }
  fixed_lit(w, 256);
}

static void stored_blocks(BitOut& w, const Bytes& d, bool last) {
  size_t i = 0;
  do {
    size_t k = d.size() - i < 65535 ? d.size() - i : 65535;
    w.bits(last && i + k == d.size() ? 1 : 0, 1);
    w.bits(0, 2);
    w.align();
    w.bits((uint32_t)k, 16);
    w.bits((uint32_t)k ^ 0xFFFFu, 16);
    for (size_t j = 0; j < k; j++) w.bits(d[i + j], 8);
    i += k;
  } while (i < d.size());
}

// kind 0: stored, 1: fixed, 2: fixed, an empty stored block (a sync flush)
// and stored, in three blocks
static Bytes deflate_raw(const Bytes& d, int kind) {
  BitOut w;
  if (kind == 0) {
    stored_blocks(w, d, true);
  } else if (kind == 1) {
    fixed_block(w, d, true);
  } else {
    size_t half = d.size() / 2;
    fixed_block(w, Bytes(d.begin(), d.begin() + half), false);
    stored_blocks(w, Bytes(), false);
    stored_blocks(w, Bytes(d.begin() + half, d.end()), true);
  }
  w.align();
  return w.out;
}

static void put_le32(Bytes& b, uint32_t v) {
  for (int i = 0; i < 4; i++) b.push_back((uint8_t)(v >> (8 * i)));
}

static Bytes gzip_wrap(const Bytes& raw, const Bytes& orig, bool fields = false) {
  Bytes p = {0x1f, 0x8b, 8, (uint8_t)(fields ? 2 | 4 | 8 | 16 : 0), 0, 0, 0, 0, 0, 3};
  if (fields) {
    const uint8_t more[] = {3, 0, 'x', 'y', 'z', 'n', 'a', 'm', 'e', 0, 'c', 0, 0x12, 0x34};
    p.insert(p.end(), more, more + sizeof(more));
  }
  p.insert(p.end(), raw.begin(), raw.end());
  put_le32(p, lsinfl::crc32(orig.data(), (int64_t)orig.size()));
  put_le32(p, (uint32_t)orig.size());
  return p;
}

static Bytes zlib_wrap(const Bytes& raw, const Bytes& orig) {
  Bytes p = {0x78, 0x9c};
  p.insert(p.end(), raw.begin(), raw.end());
  uint32_t a = lsinfl::adler32(orig.data(), (int64_t)orig.size());
  for (int i = 3; i >= 0; i--) p.push_back((uint8_t)(a >> (8 * i)));
  return p;
}

static bool round_trip(const char* name, const Bytes& orig) {
  bool ok = true;
  for (int kind = 0; kind < 3; kind++) {
    Bytes raw = deflate_raw(orig, kind), out;
    Bytes pages[3] = {gzip_wrap(raw, orig), zlib_wrap(raw, orig),
                      gzip_wrap(raw, orig, true)};
    for (const Bytes& page : pages) {
      if (!decode_exact(page, orig.size(), &out) || out != orig) {
        std::printf("FAIL %s/%zu kind %d: round trip\n", name, orig.size(), kind);
        ok = false;
      }
      if (decode_exact(page, orig.size() + 1, nullptr) ||
          (!orig.empty() && decode_exact(page, orig.size() - 1, nullptr))) {
        std::printf("FAIL %s/%zu kind %d: wrong page size accepted\n", name,
                    orig.size(), kind);
        ok = false;
      }
    }
    if (!decode_exact(raw, orig.size(), &out, true) || out != orig) {
      std::printf("FAIL %s/%zu kind %d: bare stream\n", name, orig.size(), kind);
      ok = false;
    }
  }
  return ok;
}

// every truncation, four replacements of every byte, trailing garbage
static void damage(const Bytes& page, size_t n) {
  for (size_t cut = 0; cut < page.size(); cut++)
    decode_exact(Bytes(page.begin(), page.begin() + cut), n, nullptr);
  for (size_t i = 0; i < page.size(); i++) {
    static const uint8_t kFlip[] = {0x01, 0x80, 0xFF, 0x10};
    for (uint8_t f : kFlip) {
      Bytes m = page, out;
      m[i] ^= f;
      decode_exact(m, n, &out);
    }
  }
  for (size_t extra = 1; extra <= 16; extra++) {
    Bytes m = page;
    for (size_t k = 0; k < extra; k++) m.push_back((uint8_t)rnd());
    decode_exact(m, n, nullptr);
  }
}

// the table of lens as one lane builds it, and as 64 lanes do
static bool lanes_agree(int type, const uint8_t* lens, int n, int cap, int root) {
  std::vector<uint32_t> one((size_t)cap, 0xFFFFFFFFu), many((size_t)cap, 0xFFFFFFFFu);
  lsinfl::Work w;
  bool ok1 = lsinfl::build_table(type, lens, n, one.data(), cap, root, w, 0, 1);
  bool okn = true;
  for (int lane = 0; lane < 64; lane++)
    okn &= lsinfl::build_table(type, lens, n, many.data(), cap, root, w, lane, 64);
  return ok1 && okn && one == many;
}

int main() {
  bool ok = true;
  const uint8_t nine[] = {'1', '2', '3', '4', '5', '6', '7', '8', '9'};
  ok &= expect(lsinfl::crc32(nine, 9) == 0xCBF43926u, "crc32 check value");
  ok &= expect(lsinfl::adler32((const uint8_t*)"Wikipedia", 9) == 0x11E60398u,
               "adler32 check value");

  const size_t N = 131072;
  Bytes ids(N), i32(N), noise(N), eq(N, 7), per(N);
  for (size_t i = 0; i < N / 8; i++) {
    uint64_t id = 1000000 + i;
    uint32_t s0 = rnd() % 100, s1 = rnd() % 100;
    std::memcpy(&ids[8 * i], &id, 8);
    std::memcpy(&i32[8 * i], &s0, 4);
    std::memcpy(&i32[8 * i + 4], &s1, 4);
  }
  for (size_t i = 0; i < N; i++) {
    noise[i] = (uint8_t)rnd();
    per[i] = (uint8_t)(i % 13);
  }
  // a second copy 32768 behind the first: matches at the largest distance
  Bytes far(noise.begin(), noise.begin() + 32768);
  far.insert(far.end(), noise.begin(), noise.begin() + 32768);
  far.insert(far.end(), noise.begin(), noise.begin() + 32768);

  struct Src { const char* name; const Bytes* b; };
  const Src srcs[] = {{"ids", &ids}, {"i32", &i32}, {"noise", &noise},
                      {"equal", &eq}, {"period13", &per}, {"far", &far}};
  for (const Src& s : srcs) {
    for (size_t n = 0; n <= 20; n++)
      ok &= round_trip(s.name, Bytes(s.b->begin(), s.b->begin() + n));
    static const size_t kLens[] = {63, 64, 65, 258, 259, 4096, 65535, 65536, 98304};
    for (size_t n : kLens)
      if (n <= s.b->size()) ok &= round_trip(s.name, Bytes(s.b->begin(), s.b->begin() + n));
  }
  {
    Bytes raw = deflate_raw(far, 1);
    ok &= expect(raw.size() < 60000 && g_max_len == 258 && g_max_dist == 32768,
                 "the far copy becomes matches of length 258 at distance 32768");
  }

  // two members; a member of nothing in between
  {
    Bytes a(ids.begin(), ids.begin() + 1000), b(i32.begin(), i32.begin() + 777), none;
    Bytes page = gzip_wrap(deflate_raw(a, 1), a);
    Bytes pn = gzip_wrap(deflate_raw(none, 1), none), pb = gzip_wrap(deflate_raw(b, 2), b);
    page.insert(page.end(), pn.begin(), pn.end());
    page.insert(page.end(), pb.begin(), pb.end());
    Bytes ab = a, out;
    ab.insert(ab.end(), b.begin(), b.end());
    ok &= expect(decode_exact(page, ab.size(), &out) && out == ab, "three members");
    damage(page, ab.size());
  }

  // recorded streams
  {
    Bytes text, out;
    for (int i = 0; i < 80; i++) {
      char buf[32];
      int k = std::snprintf(buf, sizeof buf, "col_%d=%d;", i % 7, i * i % 1000);
      text.insert(text.end(), buf, buf + k);
    }
    Bytes dyn(kDynamicPage, kDynamicPage + sizeof kDynamicPage);
    ok &= expect(decode_exact(dyn, text.size(), &out) && out == text, "zlib level 9 page");
    long before = g_failed;
    damage(dyn, text.size());
    ok &= expect(g_failed - before > (long)dyn.size(), "damaged pages are refused");

    struct Rec { const char* name; const uint8_t* p; size_t n, out_n; uint32_t crc; };
    const Rec recs[] = {
        {"15-bit code", kRaw15Bit, sizeof kRaw15Bit, 305, 0x66461414u},
        {"single distance code", kRawSingleDist, sizeof kRawSingleDist, 8, 0xbf848046u},
        {"repeat across HLIT", kRawRepeatAcross, sizeof kRawRepeatAcross, 17, 0x61933e27u},
    };
    for (const Rec& r : recs) {
      Bytes raw(r.p, r.p + r.n);
      ok &= expect(decode_exact(raw, r.out_n, &out, true) &&
                       lsinfl::crc32(out.data(), (int64_t)out.size()) == r.crc, r.name);
      damage(gzip_wrap(raw, out), r.out_n);
    }
  }

  // damaged stored, fixed and zlib pages
  {
    Bytes part(i32.begin(), i32.begin() + 600);
    for (int kind = 0; kind < 3; kind++) {
      damage(gzip_wrap(deflate_raw(part, kind), part), part.size());
      damage(zlib_wrap(deflate_raw(part, kind), part), part.size());
    }
    damage(gzip_wrap(deflate_raw(part, 1), part, true), part.size());
  }

  // the lanes' split of the table fill
  {
    uint8_t lens[320];
    for (int s = 0; s < 288; s++) lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    ok &= expect(lanes_agree(lsinfl::T_LENS, lens, 288, lsinfl::kLitCap, lsinfl::kLitRoot),
                 "lanes: fixed literal/length code");
    for (int s = 0; s < 32; s++) lens[s] = 5;
    ok &= expect(lanes_agree(lsinfl::T_DISTS, lens, 32, lsinfl::kDistCap, lsinfl::kDistRoot),
                 "lanes: fixed distance code");
    // lengths 1, 2, ..., 14, 15, 15: sub-tables of every depth
    for (int s = 0; s < 15; s++) lens[s] = (uint8_t)(s + 1);
    for (int s = 15; s < 256; s++) lens[s] = 0;
    lens[256] = 15;
    ok &= expect(lanes_agree(lsinfl::T_LENS, lens, 257, lsinfl::kLitCap, lsinfl::kLitRoot),
                 "lanes: 15-bit literal/length code");
    ok &= expect(lanes_agree(lsinfl::T_DISTS, lens, 15 + 1, lsinfl::kDistCap, lsinfl::kDistRoot) == false,
                 "an incomplete distance code is refused");
    lens[15] = 15;
    ok &= expect(lanes_agree(lsinfl::T_DISTS, lens, 16, lsinfl::kDistCap, lsinfl::kDistRoot),
                 "lanes: 15-bit distance code");
    uint8_t one[4] = {0, 1, 0, 0}, none[4] = {0, 0, 0, 0};
    ok &= expect(lanes_agree(lsinfl::T_DISTS, one, 4, lsinfl::kDistCap, lsinfl::kDistRoot),
                 "lanes: one 1-bit distance code");
    ok &= expect(lanes_agree(lsinfl::T_DISTS, none, 4, lsinfl::kDistCap, lsinfl::kDistRoot),
                 "lanes: no distance code");
    ok &= expect(!lanes_agree(lsinfl::T_LENS, one, 4, lsinfl::kLitCap, lsinfl::kLitRoot),
                 "an incomplete literal/length code is refused");
    // random complete codes: split the unit interval until 286 / 30 leaves
    for (int round = 0; round < 200; round++) {
      int want = round % 2 ? 30 : 286, type = round % 2 ? lsinfl::T_DISTS : lsinfl::T_LENS;
      std::vector<uint8_t> l = {1, 1};
      while ((int)l.size() < want) {
        size_t k = rnd() % l.size();
        if (l[k] >= 15) continue;
        l[k]++;
        l.push_back(l[k]);
      }
      ok &= expect(lanes_agree(type, l.data(), (int)l.size(),
                               round % 2 ? lsinfl::kDistCap : lsinfl::kLitCap,
                               round % 2 ? lsinfl::kDistRoot : lsinfl::kLitRoot),
                   "lanes: random complete code");
    }
  }

  std::printf("%s decodes=%ld refused=%ld\n", ok ? "OK" : "FAIL", g_runs, g_failed);
  return ok ? 0 : 1;
}
