// Bounds check of the Huffman-only page classifier and the lane-parallel
// Huffman decode (csrc/cpp/huf_par.h) — built with
// -fsanitize=address,undefined by
// tests/test_huf_par.py::test_huf_par_sanitizer_clean. Every frame the
// classifier accepts, and 200 seeded one-byte corruptions of each, go
// through huf_only_frame and huf_par_decode with input and output in
// exactly-sized heap buffers, so any read or write past either end is a
// sanitizer report. A corrupted frame may fail or decode to other bytes;
// an intact one must decode to its original. The per-lane steps under test
// are the ones the GPU kernel runs (csrc/hip/zstd_huf.hip), which has no
// sanitizer of its own.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../huf_par.h"

extern "C" {
size_t ZSTD_compress(void* dst, size_t dstCapacity, const void* src,
                     size_t srcSize, int compressionLevel);
size_t ZSTD_compressBound(size_t srcSize);
unsigned ZSTD_isError(size_t code);
}

using Bytes = std::vector<uint8_t>;

static lszstd::HufParCtx* g_ctx = new lszstd::HufParCtx();
static long g_runs = 0, g_accepted = 0, g_failed = 0;

static uint32_t g_lcg = 2463534242u;
static uint32_t rnd() {
  g_lcg = g_lcg * 1664525u + 1013904223u;
  return g_lcg >> 8;
}
static double unif() { return (rnd() + 1.0) / 16777217.0; }

// classifier, then decode, both on exactly-sized copies
static bool decode_exact(const Bytes& frame, size_t rs, int lanes, Bytes* out) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[frame.size()]), dst(new uint8_t[rs]);
  std::memcpy(in.get(), frame.data(), frame.size());
  lszstd::HufOnly ho;
  bool accepted = lszstd::huf_only_frame(in.get(), (int64_t)frame.size(), (int64_t)rs, ho);
  bool ok = lszstd::huf_par_decode(in.get(), (int64_t)frame.size(), dst.get(),
                                   (int64_t)rs, lanes, *g_ctx);
  g_runs++;
  if (ok && !accepted) {
    std::printf("FAIL: decoded a frame the classifier rejects\n");
    std::exit(1);
  }
  if (ok && out) out->assign(dst.get(), dst.get() + rs);
  return ok;
}

static bool torture(const char* name, const Bytes& orig) {
  Bytes frame(ZSTD_compressBound(orig.size()));
  size_t r = ZSTD_compress(frame.data(), frame.size(), orig.data(), orig.size(), 1);
  if (ZSTD_isError(r)) std::abort();
  frame.resize(r);
  lszstd::HufOnly ho;
  if (!lszstd::huf_only_frame(frame.data(), (int64_t)frame.size(),
                              (int64_t)orig.size(), ho))
    return true;  // raw block or sequences: not this decoder's page
  g_accepted++;
  static const int kLanes[] = {1, 3, 64, 256};
  for (int lanes : kLanes) {
    Bytes out;
    if (!decode_exact(frame, orig.size(), lanes, &out) || out != orig) {
      std::printf("FAIL %s/%zu: intact frame, %d lanes\n", name, orig.size(), lanes);
      return false;
    }
  }
  for (int k = 0; k < 200; k++) {
    Bytes m = frame;
    size_t i = rnd() % m.size();
    m[i] ^= (uint8_t)(1u << (rnd() % 8));
    if (!decode_exact(m, orig.size(), 64, nullptr)) g_failed++;
  }
  for (size_t cut = 1; cut < frame.size() && cut <= 16; cut++) {
    Bytes m(frame.begin(), frame.end() - cut);
    if (decode_exact(m, orig.size(), 64, nullptr)) {
      std::printf("FAIL %s/%zu: truncated frame decodes\n", name, orig.size());
      return false;
    }
  }
  return true;
}

int main() {
  const size_t N = 131072;
  Bytes f64(N), f32(N), i64(N), geo(N), u16(N), u40(N);
  for (size_t i = 0; i < N / 8; i++) {
    double g = std::sqrt(-2.0 * std::log(unif())) * std::cos(6.283185307179586 * unif());
    float gf = (float)(std::sqrt(-2.0 * std::log(unif())) * std::sin(6.283185307179586 * unif()));
    float gf2 = (float)(std::sqrt(-2.0 * std::log(unif())) * std::cos(6.283185307179586 * unif()));
    uint64_t v = (((uint64_t)rnd() << 24) | rnd()) % 1000000000000ull;
    std::memcpy(&f64[8 * i], &g, 8);
    std::memcpy(&f32[8 * i], &gf, 4);
    std::memcpy(&f32[8 * i + 4], &gf2, 4);
    std::memcpy(&i64[8 * i], &v, 8);
  }
  for (size_t i = 0; i < N; i++) {
    double k = std::floor(std::log(unif()) / std::log(1.0 - 0.08));
    geo[i] = (uint8_t)(k > 255 ? 255 : k);
    u16[i] = (uint8_t)(rnd() % 16);
    u40[i] = (uint8_t)(rnd() % 40);
  }
  static const size_t kLens[] = {200, 256, 300, 1000, 1021, 1022, 1023, 1024,
                                 1025, 4096, 16383, 16384, 65536, 131072};
  struct Src { const char* name; const Bytes* b; };
  const Src srcs[] = {{"f64", &f64}, {"f32", &f32}, {"i64", &i64},
                      {"geo08", &geo}, {"u16", &u16}, {"u40", &u40}};
  bool ok = true;
  for (const Src& s : srcs)
    for (size_t n : kLens)
      ok &= torture(s.name, Bytes(s.b->begin(), s.b->begin() + n));
  if (g_accepted < 40 || g_failed == 0) {
    std::printf("FAIL: %ld frames accepted, %ld corruptions failed\n", g_accepted, g_failed);
    ok = false;
  }
  std::printf("%s accepted=%ld decodes=%ld failed=%ld\n", ok ? "OK" : "FAIL",
              g_accepted, g_runs, g_failed);
  return ok ? 0 : 1;
}
