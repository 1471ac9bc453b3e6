// Bounds check of the LZ4 block codec (csrc/cpp/lz4_dec.h) — built with
// -fsanitize=address,undefined by tests/test_lz4.py::test_lz4_sanitizer_clean.
// Input and output sit in exactly-sized heap buffers, so any read or write
// past either end is a sanitizer report.
// - The encoder's blocks of the five headline column shapes (and two
//   compressible fillers) at 0 B to 128 KB decode back to their input.
// - Hand-built blocks hit the length extension bytes, an offset of zero, an
//   offset past the output, a block that ends in a match and a run of 0xFF
//   extension bytes that reaches the end of the input.
// - A 300-byte block is truncated at every length, has every byte replaced
//   by four other values and gets trailing garbage: each decode fails or
//   yields exactly the page's size.
// - Hadoop framing: one frame, three frames, a raw block, damaged headers.
// lz4_parse_seq and the bounds checks under test are the ones the GPU
// kernel runs (csrc/hip/lz4.hip), which has no sanitizer of its own.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../lz4_dec.h"

using Bytes = std::vector<uint8_t>;

static long g_runs = 0, g_failed = 0;

static uint32_t g_lcg = 2463534242u;
static uint32_t rnd() {
  g_lcg = g_lcg * 1664525u + 1013904223u;
  return g_lcg >> 8;
}
static double unif() { return (rnd() + 1.0) / 16777217.0; }

// decode on exactly-sized copies; `hadoop` picks the framed entry point
static bool decode_exact(const Bytes& block, size_t n, Bytes* out,
                         bool hadoop = false) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[block.size()]), dst(new uint8_t[n]);
  if (!block.empty()) std::memcpy(in.get(), block.data(), block.size());
  bool ok = hadoop ? lslz4::lz4_hadoop_decode(dst.get(), (int64_t)n, in.get(),
                                              (int64_t)block.size())
                   : lslz4::lz4_block_decode(dst.get(), (int64_t)n, in.get(),
                                             (int64_t)block.size());
  g_runs++;
  if (!ok) g_failed++;
  if (ok && out) out->assign(dst.get(), dst.get() + n);
  return ok;
}

static Bytes encode_exact(const Bytes& orig) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[orig.size()]);
  if (!orig.empty()) std::memcpy(in.get(), orig.data(), orig.size());
  return lslz4::lz4_block_encode(in.get(), orig.size());
}

static bool round_trip(const char* name, const Bytes& orig) {
  Bytes block = encode_exact(orig), out;
  if (!decode_exact(block, orig.size(), &out) || out != orig) {
    std::printf("FAIL %s/%zu: round trip\n", name, orig.size());
    return false;
  }
  // end-of-block rules: the closing literal run is at least 5 bytes, or
  // the whole input
  if (orig.size() < 13 && block.size() != orig.size() + 1) {
    std::printf("FAIL %s/%zu: short input is not one literal run\n", name,
                orig.size());
    return false;
  }
  // a page one byte larger or smaller is refused
  if (decode_exact(block, orig.size() + 1, nullptr) ||
      (!orig.empty() && decode_exact(block, orig.size() - 1, nullptr))) {
    std::printf("FAIL %s/%zu: wrong page size accepted\n", name, orig.size());
    return false;
  }
  return true;
}

static void put_be32(Bytes& b, uint32_t v) {
  b.push_back((uint8_t)(v >> 24));
  b.push_back((uint8_t)(v >> 16));
  b.push_back((uint8_t)(v >> 8));
  b.push_back((uint8_t)v);
}

static bool expect(bool cond, const char* what) {
  if (!cond) std::printf("FAIL: %s\n", what);
  return cond;
}

int main() {
  const size_t N = 131072;
  Bytes ids(N), f64(N), i32(N), f32(N), i64(N), eq(N, 7), per(N);
  for (size_t i = 0; i < N / 8; i++) {
    double g = std::sqrt(-2.0 * std::log(unif())) * std::cos(6.283185307179586 * unif());
    float gf = (float)unif(), gf2 = (float)(unif() * 1000.0);
    uint64_t id = 1000000 + i;
    uint64_t v = (((uint64_t)rnd() << 24) | rnd()) % 1000000000000ull;
    uint32_t s0 = rnd() % 100, s1 = rnd() % 100;
    std::memcpy(&ids[8 * i], &id, 8);
    std::memcpy(&f64[8 * i], &g, 8);
    std::memcpy(&i32[8 * i], &s0, 4);
    std::memcpy(&i32[8 * i + 4], &s1, 4);
    std::memcpy(&f32[8 * i], &gf, 4);
    std::memcpy(&f32[8 * i + 4], &gf2, 4);
    std::memcpy(&i64[8 * i], &v, 8);
  }
  for (size_t i = 0; i < N; i++) per[i] = (uint8_t)(i % 13);

  bool ok = true;
  struct Src { const char* name; const Bytes* b; };
  const Src srcs[] = {{"ids", &ids}, {"f64", &f64}, {"i32", &i32}, {"f32", &f32},
                      {"i64", &i64}, {"equal", &eq}, {"period13", &per}};
  for (const Src& s : srcs) {
    for (size_t n = 0; n <= 40; n++)
      ok &= round_trip(s.name, Bytes(s.b->begin(), s.b->begin() + n));
    static const size_t kLens[] = {200, 269, 270, 300, 1000, 4096, 65535, 65536,
                                   65537, 131072};
    for (size_t n : kLens)
      ok &= round_trip(s.name, Bytes(s.b->begin(), s.b->begin() + n));
  }
  {
    Bytes block = encode_exact(ids);
    ok &= expect(block.size() < ids.size(), "sorted ids do not compress");
  }

  // hand-built blocks
  {
    Bytes out;
    ok &= expect(decode_exact({0x00}, 0, &out), "empty page");
    ok &= expect(!decode_exact({}, 0, nullptr), "no token at all");
    // 4 literals, match offset 0
    ok &= expect(!decode_exact({0x40, 'a', 'b', 'c', 'd', 0, 0, 0x50, 1, 2, 3, 4, 5}, 13,
                               nullptr), "offset 0");
    // offset 5 with 4 bytes of output
    ok &= expect(!decode_exact({0x40, 'a', 'b', 'c', 'd', 5, 0, 0x50, 1, 2, 3, 4, 5}, 13,
                               nullptr), "offset past the output");
    // ends in a match
    ok &= expect(!decode_exact({0x40, 'a', 'b', 'c', 'd', 4, 0}, 8, nullptr),
                 "block ends in a match");
    // the same with closing literals decodes
    ok &= expect(decode_exact({0x40, 'a', 'b', 'c', 'd', 4, 0, 0x50, 1, 2, 3, 4, 5}, 13,
                              &out) && out[4] == 'a' && out[7] == 'd' && out[12] == 5,
                 "literals, match, literals");
    // literal and match extension bytes that run to the end of the input
    Bytes ff(4096, 0xFF);
    ff[0] = 0xF0;
    ok &= expect(!decode_exact(ff, 1 << 20, nullptr), "0xFF literal extension run");
    Bytes mf = {0x1F, 'x', 1, 0};
    mf.resize(4096, 0xFF);
    ok &= expect(!decode_exact(mf, 1 << 20, nullptr), "0xFF match extension run");
    // a match length that overruns the page
    ok &= expect(!decode_exact({0x1F, 'x', 1, 0, 200, 0x50, 1, 2, 3, 4, 5}, 30, nullptr),
                 "match past the page");
    // literal length 15 + 255 + 1 = 271 through ff 01
    Bytes l271 = {0xF0, 0xFF, 0x01};
    l271.resize(3 + 271, 'q');
    ok &= expect(decode_exact(l271, 271, &out) && out[270] == 'q', "literal run of 271");
  }

  // damaged 300-byte block
  {
    Bytes orig(ids.begin(), ids.begin() + 600);
    for (size_t i = 300; i < 600; i += 7) orig[i] = (uint8_t)rnd();
    Bytes block = encode_exact(orig);
    while (block.size() > 300) {  // trim the input until the block has 300 bytes
      orig.pop_back();
      block = encode_exact(orig);
    }
    ok &= expect(block.size() >= 250, "damage target is about 300 bytes");
    long before = g_failed;
    for (size_t cut = 0; cut < block.size(); cut++)
      decode_exact(Bytes(block.begin(), block.begin() + cut), orig.size(), nullptr);
    for (size_t i = 0; i < block.size(); i++) {
      static const uint8_t kFlip[] = {0x01, 0x80, 0xFF, 0x10};
      for (uint8_t f : kFlip) {
        Bytes m = block;
        m[i] ^= f;
        Bytes out;
        decode_exact(m, orig.size(), &out);
      }
    }
    for (size_t extra = 1; extra <= 16; extra++) {
      Bytes m = block;
      for (size_t k = 0; k < extra; k++) m.push_back((uint8_t)rnd());
      decode_exact(m, orig.size(), nullptr);
    }
    ok &= expect(g_failed - before > (long)block.size(), "damaged blocks are refused");
  }

  // Hadoop framing
  {
    Bytes a(ids.begin(), ids.begin() + 1000), b(i32.begin(), i32.begin() + 777),
        c(f64.begin(), f64.begin() + 50);
    Bytes ba = encode_exact(a), bb = encode_exact(b), bc = encode_exact(c), out;
    Bytes one;
    put_be32(one, (uint32_t)a.size());
    put_be32(one, (uint32_t)ba.size());
    one.insert(one.end(), ba.begin(), ba.end());
    ok &= expect(decode_exact(one, a.size(), &out, true) && out == a, "one frame");
    Bytes three = one, abc = a;
    put_be32(three, (uint32_t)b.size());
    put_be32(three, (uint32_t)bb.size());
    three.insert(three.end(), bb.begin(), bb.end());
    put_be32(three, (uint32_t)c.size());
    put_be32(three, (uint32_t)bc.size());
    three.insert(three.end(), bc.begin(), bc.end());
    abc.insert(abc.end(), b.begin(), b.end());
    abc.insert(abc.end(), c.begin(), c.end());
    ok &= expect(decode_exact(three, abc.size(), &out, true) && out == abc, "three frames");
    ok &= expect(decode_exact(ba, a.size(), &out, true) && out == a,
                 "raw block under the framed codec");
    for (size_t i = 0; i < 24 && i < three.size(); i++) {
      static const uint8_t kFlip[] = {0x01, 0x80, 0xFF};
      for (uint8_t f : kFlip) {
        Bytes m = three;
        m[i] ^= f;
        decode_exact(m, abc.size(), nullptr, true);
      }
    }
    for (size_t cut = 0; cut < three.size(); cut += 3)
      decode_exact(Bytes(three.begin(), three.begin() + cut), abc.size(), nullptr, true);
  }

  std::printf("%s decodes=%ld refused=%ld\n", ok ? "OK" : "FAIL", g_runs, g_failed);
  return ok ? 0 : 1;
}
