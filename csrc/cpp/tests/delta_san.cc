// Bounds and overflow check of the delta.h decoders — built with
// -fsanitize=address,undefined by
// tests/test_parquet_encodings.py::test_delta_sanitizer_clean. A small
// test-only encoder writes DELTA_BINARY_PACKED streams in any block
// layout (pyarrow writes int64 as 256/4 only; parquet-mr writes 128/4),
// DELTA_LENGTH_BYTE_ARRAY and DELTA_BYTE_ARRAY. Each valid stream must
// round-trip. Then every proper prefix of it, and it with each single byte
// cleared, set and inverted (each bit flipped in the first 64 bytes, where
// the headers and width bytes sit) goes through the walk and the decoders in
// an exactly-sized heap buffer: they may return or throw anything, a
// sanitizer report fails the run, and every miniblock the walk reports
// must lie wholly inside the buffer — the property the GPU kernel
// (csrc/hip/delta.hip) relies on.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "../delta.h"

using Bytes = std::vector<uint8_t>;
using namespace lakesoul;

static long g_runs = 0;
static bool g_ok = true;

static void fail(const std::string& what) {
  std::printf("FAIL %s\n", what.c_str());
  g_ok = false;
}

// ---- test-only encoder ------------------------------------------------ //

static void put_uleb(Bytes& b, uint64_t v) {
  while (v >= 0x80) {
    b.push_back((uint8_t)(v | 0x80));
    v >>= 7;
  }
  b.push_back((uint8_t)v);
}

static void put_zigzag(Bytes& b, int64_t v) {
  put_uleb(b, ((uint64_t)v << 1) ^ (uint64_t)(v >> 63));
}

// sign-extend the low `bits` of v
static int64_t sext(uint64_t v, int bits) {
  if (bits == 64) return (int64_t)v;
  uint64_t m = 1ull << (bits - 1);
  v &= (1ull << bits) - 1;
  return (int64_t)((v ^ m) - m);
}

static int bits_needed(uint64_t v) {
  int n = 0;
  while (v) {
    n++;
    v >>= 1;
  }
  return n;
}

static Bytes dbp_encode(const std::vector<uint64_t>& vals, int type_bits,
                        uint64_t block, uint64_t miniblocks) {
  Bytes b;
  const uint64_t tmask = type_bits == 64 ? ~0ull : (1ull << type_bits) - 1;
  const uint64_t vpm = block / miniblocks;
  put_uleb(b, block);
  put_uleb(b, miniblocks);
  put_uleb(b, vals.size());
  put_zigzag(b, vals.empty() ? 0 : sext(vals[0], type_bits));
  std::vector<int64_t> deltas;
  for (size_t i = 1; i < vals.size(); i++)
    deltas.push_back(sext(vals[i] - vals[i - 1], type_bits));
  for (size_t b0 = 0; b0 < deltas.size(); b0 += block) {
    size_t bn = std::min<size_t>(block, deltas.size() - b0);
    int64_t mn = deltas[b0];
    for (size_t i = 0; i < bn; i++) mn = std::min(mn, deltas[b0 + i]);
    put_zigzag(b, mn);
    std::vector<int> widths(miniblocks, 0);
    for (uint64_t m = 0; m < miniblocks; m++) {
      uint64_t mx = 0;
      for (uint64_t i = m * vpm; i < (m + 1) * vpm && i < bn; i++)
        mx = std::max(mx, ((uint64_t)deltas[b0 + i] - (uint64_t)mn) & tmask);
      widths[m] = bits_needed(mx);
    }
    for (int w : widths) b.push_back((uint8_t)w);
    for (uint64_t m = 0; m < miniblocks && m * vpm < bn; m++) {
      int w = widths[m];
      Bytes mbuf((size_t)(vpm * w / 8), 0);  // padded to full size
      for (uint64_t i = 0; i < vpm && m * vpm + i < bn; i++) {
        uint64_t rel = ((uint64_t)deltas[b0 + m * vpm + i] - (uint64_t)mn) & tmask;
        for (int k = 0; k < w; k++)
          if ((rel >> k) & 1) {
            uint64_t bit = i * w + k;
            mbuf[bit >> 3] |= (uint8_t)(1u << (bit & 7));
          }
      }
      b.insert(b.end(), mbuf.begin(), mbuf.end());
    }
  }
  return b;
}

static Bytes dlba_encode(const std::vector<std::string>& v) {
  std::vector<uint64_t> lens;
  for (auto& s : v) lens.push_back(s.size());
  Bytes b = dbp_encode(lens, 32, 128, 4);
  for (auto& s : v) b.insert(b.end(), s.begin(), s.end());
  return b;
}

static Bytes dba_encode(const std::vector<std::string>& v) {
  std::vector<uint64_t> pre;
  std::vector<std::string> suf;
  std::string prev;
  for (auto& s : v) {
    size_t p = 0;
    while (p < s.size() && p < prev.size() && s[p] == prev[p]) p++;
    pre.push_back(p);
    suf.push_back(s.substr(p));
    prev = s;
  }
  Bytes b = dbp_encode(pre, 32, 128, 4);
  Bytes t = dlba_encode(suf);
  b.insert(b.end(), t.begin(), t.end());
  return b;
}

static Bytes plain_strings(const std::vector<std::string>& v) {
  Bytes b;
  for (auto& s : v) {
    uint32_t l = (uint32_t)s.size();
    b.insert(b.end(), (uint8_t*)&l, (uint8_t*)&l + 4);
    b.insert(b.end(), s.begin(), s.end());
  }
  return b;
}

// ---- decoders on an exactly-sized heap copy --------------------------- //

enum Kind { K_DBP32, K_DBP64, K_DLBA, K_DBA };

// true when the decoder returned (did not throw); out gets its output
static bool run_decoder(Kind k, const uint8_t* src, size_t len, int64_t n,
                        Bytes& out, size_t* used = nullptr) {
  std::unique_ptr<uint8_t[]> in(new uint8_t[len ? len : 1]);
  if (len) std::memcpy(in.get(), src, len);
  const uint8_t* p = in.get();
  g_runs++;
  // the walk: every reported miniblock inside the buffer
  if (k == K_DBP32 || k == K_DBP64) {
    DeltaHeader h;
    try {
      delta_walk(p, len, k == K_DBP32 ? 32 : 64, (uint64_t)n, h,
                 [&](const DeltaMiniblock& m) {
        uint64_t span = h.values_per_miniblock * (uint64_t)m.bit_width;
        if (m.bit_off < 0 || m.bit_width < 0 ||
            m.bit_width > (k == K_DBP32 ? 32 : 64) || m.n <= 0 ||
            (uint64_t)m.n > h.values_per_miniblock ||
            (uint64_t)m.bit_off + span > (uint64_t)len * 8)
          fail("walk reported a miniblock outside the buffer");
      });
    } catch (const std::exception&) {
    }
  }
  try {
    size_t u = 0;
    switch (k) {
      case K_DBP32: u = delta_binary_decode<int32_t>(p, len, n, out); break;
      case K_DBP64: u = delta_binary_decode<int64_t>(p, len, n, out); break;
      case K_DLBA: u = delta_length_byte_array_decode(p, len, n, out); break;
      case K_DBA: u = delta_byte_array_decode(p, len, n, out); break;
    }
    if (u > len) fail("decoder consumed more than the buffer");
    if (used) *used = u;
    return true;
  } catch (const std::exception&) {
    return false;
  }
}

static void torture(const char* name, Kind k, const Bytes& s, int64_t n,
                    const Bytes& want) {
  Bytes got;
  size_t used = 0;
  if (!run_decoder(k, s.data(), s.size(), n, got, &used) || got != want ||
      used != s.size()) {
    fail(std::string(name) + ": intact stream does not round-trip");
    return;
  }
  for (size_t len = 0; len < s.size(); len++) {
    Bytes o;
    run_decoder(k, s.data(), len, n, o);
  }
  for (size_t i = 0; i < s.size(); i++) {
    // headers, min deltas and width bytes of the first block: every bit;
    // further in: the byte cleared, set and inverted
    uint8_t repl[10] = {0x00, 0xFF, (uint8_t)~s[i]};
    int nrepl = 3;
    if (i < 64)
      for (int b = 1; b < 8; b++) repl[nrepl++] = (uint8_t)(s[i] ^ (1u << b));
    for (int q = 0; q < nrepl; q++) {
      uint8_t r = repl[q];
      if (r == s[i]) continue;
      Bytes m = s, o;
      m[i] = r;
      run_decoder(k, m.data(), m.size(), n, o);
    }
  }
}

static Bytes raw_of(const std::vector<uint64_t>& v, int type_bits) {
  Bytes b;
  for (uint64_t x : v) {
    if (type_bits == 32) {
      uint32_t t = (uint32_t)x;
      b.insert(b.end(), (uint8_t*)&t, (uint8_t*)&t + 4);
    } else {
      b.insert(b.end(), (uint8_t*)&x, (uint8_t*)&x + 8);
    }
  }
  return b;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

int main() {
  const uint64_t I64MAX = 0x7FFFFFFFFFFFFFFFull, I64MIN = 0x8000000000000000ull;
  const uint64_t I32MAX = 0x7FFFFFFFull, I32MIN = 0xFFFFFFFF80000000ull;
  struct Layout { uint64_t block, mbs; };
  const Layout layouts[] = {{128, 4}, {256, 4}};
  const size_t counts[] = {1, 2, 33, 34, 65, 66, 129, 130, 257, 258};
  for (int type_bits : {32, 64}) {
    const uint64_t tmax = type_bits == 32 ? I32MAX : I64MAX;
    const uint64_t tmin = type_bits == 32 ? I32MIN : I64MIN;
    for (const Layout& L : layouts) {
      for (size_t n : counts) {
        std::vector<std::vector<uint64_t>> sets(6);
        for (size_t i = 0; i < n; i++) {
          sets[0].push_back(i);                      // arange: tiny widths
          sets[1].push_back(7);                      // constant: width 0
          sets[2].push_back((uint64_t)i * i * 1000); // widths grow
          sets[3].push_back(i % 2 ? tmax : 0);       // full-width miniblock
          sets[4].push_back(i % 2 ? tmax : tmin);    // wraparound, width 2
          sets[5].push_back(type_bits == 32 ? (uint64_t)sext(rnd(), 32) : rnd());
        }
        for (size_t si = 0; si < sets.size(); si++) {
          char name[96];
          std::snprintf(name, sizeof name, "dbp%d %llu/%llu n=%zu set=%zu",
                        type_bits, (unsigned long long)L.block,
                        (unsigned long long)L.mbs, n, si);
          Bytes s = dbp_encode(sets[si], type_bits, L.block, L.mbs);
          torture(name, type_bits == 32 ? K_DBP32 : K_DBP64, s, (int64_t)n,
                  raw_of(sets[si], type_bits));
        }
      }
    }
  }
  // widths the encoder must have produced: 64 / 32 and 2 (checked on the
  // first block's width bytes so the sets above cannot quietly degrade)
  {
    std::vector<uint64_t> v;
    for (int i = 0; i < 66; i++) v.push_back(i % 2 ? I64MAX : 0);
    Bytes s = dbp_encode(v, 64, 128, 4);
    DeltaHeader h;
    int maxw = 0;
    delta_walk(s.data(), s.size(), 64, 66, h,
               [&](const DeltaMiniblock& m) { maxw = std::max(maxw, (int)m.bit_width); });
    if (maxw != 64) fail("no 64-bit miniblock in the [0, INT64_MAX] stream");
    for (auto& x : v) x = x ? I64MAX : I64MIN;
    s = dbp_encode(v, 64, 128, 4);
    maxw = 0;
    delta_walk(s.data(), s.size(), 64, 66, h,
               [&](const DeltaMiniblock& m) { maxw = std::max(maxw, (int)m.bit_width); });
    if (maxw != 2) fail("[INT64_MIN, INT64_MAX] stream is not width 2");
  }

  // strings
  std::vector<std::vector<std::string>> ssets;
  ssets.push_back({""});
  ssets.push_back({"", "", ""});
  ssets.push_back({std::string(5000, 'x')});
  {
    std::vector<std::string> keys, mixed;
    for (int i = 0; i < 70; i++) {
      char k[64];
      std::snprintf(k, sizeof k, "tenant/0001/region/eu/key-%06d", i * 37);
      keys.push_back(k);
      mixed.push_back(i % 3 ? std::string((size_t)(i % 11), (char)('a' + i % 26))
                            : std::string("\xe4\xbd\xa0\xe5\xa5\xbd-") + k);
    }
    ssets.push_back(keys);
    ssets.push_back(mixed);
  }
  for (size_t si = 0; si < ssets.size(); si++) {
    char name[64];
    std::snprintf(name, sizeof name, "dlba set=%zu", si);
    Bytes want = plain_strings(ssets[si]);
    Bytes s = dlba_encode(ssets[si]);
    if (s.size() > 6000) {
      // the 5000-byte value: round-trip and truncations only
      Bytes got;
      if (!run_decoder(K_DLBA, s.data(), s.size(), (int64_t)ssets[si].size(), got) ||
          got != want)
        fail(std::string(name) + ": no round-trip");
      s = dba_encode(ssets[si]);
      got.clear();
      if (!run_decoder(K_DBA, s.data(), s.size(), (int64_t)ssets[si].size(), got) ||
          got != want)
        fail(std::string(name) + ": no round-trip (dba)");
      continue;
    }
    torture(name, K_DLBA, s, (int64_t)ssets[si].size(), want);
    std::snprintf(name, sizeof name, "dba set=%zu", si);
    torture(name, K_DBA, dba_encode(ssets[si]), (int64_t)ssets[si].size(), want);
  }
  {
    Bytes s = dlba_encode(ssets[2]), o;
    for (size_t len = 0; len < 64; len++) run_decoder(K_DLBA, s.data(), len, 1, o);
    s = dba_encode(ssets[2]);
    for (size_t len = 0; len < 64; len++) run_decoder(K_DBA, s.data(), len, 1, o);
  }

  // BYTE_STREAM_SPLIT: transpose round-trip, short pages throw
  for (int es : {4, 8}) {
    for (int64_t n : {1, 63, 64, 65}) {
      Bytes plain((size_t)n * es), split((size_t)n * es), got;
      for (auto& b : plain) b = (uint8_t)rnd();
      for (int64_t i = 0; i < n; i++)
        for (int k = 0; k < es; k++) split[(size_t)k * n + i] = plain[(size_t)i * es + k];
      std::unique_ptr<uint8_t[]> in(new uint8_t[split.size()]);
      std::memcpy(in.get(), split.data(), split.size());
      byte_stream_split_decode(in.get(), split.size(), n, es, got);
      if (got != plain) fail("byte-stream-split does not round-trip");
      bool threw = false;
      try {
        Bytes o;
        byte_stream_split_decode(in.get(), split.size() - 1, n, es, o);
      } catch (const std::exception&) {
        threw = true;
      }
      if (!threw) fail("byte-stream-split accepted a short page");
    }
  }

  std::printf("%s: %ld decoder runs\n", g_ok ? "OK" : "FAILED", g_runs);
  return g_ok ? 0 : 1;
}
