// Bounds check of the zstd decoder on damaged input — built with
// -fsanitize=address,undefined by
// tests/test_zstd_dec.py::test_parse_bounds_sanitizer_clean. Every proper
// prefix of each frame, and each frame with one of its first 64 bytes
// replaced, goes through lszstd::decode with input and output in
// exactly-sized heap buffers, so any read or write past either end is a
// sanitizer report. Any return value is fine. The parse functions under
// test are the ones the GPU kernel runs (csrc/hip/zstd.hip), which has no
// sanitizer of its own.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../zstd_dec.h"

extern "C" {
size_t ZSTD_compress(void* dst, size_t dstCapacity, const void* src,
                     size_t srcSize, int compressionLevel);
size_t ZSTD_compressBound(size_t srcSize);
unsigned ZSTD_isError(size_t code);
}

using Bytes = std::vector<uint8_t>;

static lszstd::Ctx* g_ctx = new lszstd::Ctx();
static long g_runs = 0;

static int64_t decode_exact(const uint8_t* src, size_t n, size_t cap) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[n]), out(new uint8_t[cap]);
  std::memcpy(in.get(), src, n);
  g_runs++;
  return lszstd::decode(in.get(), (int64_t)n, out.get(), (int64_t)cap, g_ctx);
}

static bool torture(const char* name, const Bytes& frame, size_t cap) {
  if (frame.size() > 4096) {
    std::printf("FAIL %s: frame is %zu bytes, want <= 4096\n", name, frame.size());
    return false;
  }
  if (decode_exact(frame.data(), frame.size(), cap) != (int64_t)cap) {
    std::printf("FAIL %s: intact frame does not decode to %zu bytes\n", name, cap);
    return false;
  }
  for (size_t len = 0; len < frame.size(); len++)
    decode_exact(frame.data(), len, cap);
  for (size_t i = 0; i < frame.size() && i < 64; i++) {
    const uint8_t repl[3] = {0x00, 0xFF, (uint8_t)(frame[i] ^ 0x80)};
    for (uint8_t r : repl) {
      Bytes m = frame;
      m[i] = r;
      decode_exact(m.data(), m.size(), cap);
    }
  }
  return true;
}

static Bytes from_hex(const char* h) {
  Bytes b;
  for (; h[0] && h[1]; h += 2) b.push_back((uint8_t)std::stoi(std::string(h, 2), nullptr, 16));
  return b;
}

static Bytes compress(const Bytes& p, int level) {
  Bytes out(ZSTD_compressBound(p.size()));
  size_t r = ZSTD_compress(out.data(), out.size(), p.data(), p.size(), level);
  if (ZSTD_isError(r)) std::abort();
  out.resize(r);
  return out;
}

int main() {
  bool ok = true;
  // RLE literals with the 1-, 2- and 3-byte header (tests/zstd_corpus.py)
  ok &= torture("rle_lit_1", from_hex("28b52ffd20141d0000a15a00"), 20);
  ok &= torture("rle_lit_2", from_hex("28b52ffda02c010000250000c5125a00"), 300);
  ok &= torture("rle_lit_3", from_hex("28b52ffda0881300002d00008d38015a00"), 5000);

  uint32_t lcg = 12345;
  auto rnd = [&](uint32_t m) {
    lcg = lcg * 1664525u + 1013904223u;
    return (lcg >> 8) % m;
  };
  static const char* const kWords[] = {"lake", "soul", "gpu", "zstd", "merge"};
  Bytes text, small8, i32, noise, run(5000, 'x');
  while (text.size() < 12000) {
    for (const char* w = kWords[rnd(5)]; *w; w++) text.push_back((uint8_t)*w);
    text.push_back(' ');
  }
  for (int i = 0; i < 3000; i++) small8.push_back((uint8_t)rnd(8));
  for (int i = 0; i < 1500; i++) {
    uint32_t v = rnd(500);
    for (int b = 0; b < 4; b++) i32.push_back((uint8_t)(v >> (8 * b)));
  }
  for (int i = 0; i < 2000; i++) noise.push_back((uint8_t)rnd(256));
  ok &= torture("text_l3", compress(text, 3), text.size());
  ok &= torture("text_l9", compress(text, 9), text.size());
  ok &= torture("small8_l1", compress(small8, 1), small8.size());
  ok &= torture("i32_l1", compress(i32, 1), i32.size());
  ok &= torture("i32_l9", compress(i32, 9), i32.size());
  ok &= torture("noise_l1", compress(noise, 1), noise.size());
  ok &= torture("run_l1", compress(run, 1), run.size());
  std::printf("%s decodes=%ld\n", ok ? "OK" : "FAIL", g_runs);
  return ok ? 0 : 1;
}
