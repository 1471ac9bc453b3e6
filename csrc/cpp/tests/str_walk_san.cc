// Bounds check of the GPU string route's host code: the two prefix walks
// (csrc/cpp/str_walk.h) and the host twins of the segment copy
// (csrc/cpp/str_seg.h) — built with -fsanitize=address,undefined by
// tests/test_string_route.py::test_str_walk_sanitizer_clean. Every input and
// output sits in an exactly-sized heap buffer, so any read or write past
// either end is a sanitizer report.
// - Valid streams (lengths 0..17 at every phase of a word, a 70,000-byte
//   value, 5,000 empties in a row, no values at all) walk to the expected
//   offsets, and the twins give back the values.
// - Damaged streams: a prefix past the end, a length past the end, one value
//   too few, trailing bytes, a dictionary page shorter than its entry count.
//   Each is refused.
// - A valid stream truncated at every length is refused at every length.
// - The twins on tables that do not fit their buffers (offsets past the raw
//   stream, an index equal to the dictionary size, INT32_MAX, a negative
//   index, a dictionary offset past the bytes) read nothing outside.
// lsseg::owner / dict_row_len / the delta functions are the ones the GPU
// kernel runs (csrc/hip/strings.hip), which has no sanitizer of its own.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../str_seg.h"
#include "../str_walk.h"

using Bytes = std::vector<uint8_t>;
using Values = std::vector<Bytes>;

static long g_walks = 0, g_refused = 0;

static uint32_t g_lcg = 2463534242u;
static uint32_t rnd() {
  g_lcg = g_lcg * 1664525u + 1013904223u;
  return g_lcg >> 8;
}

static bool expect(bool cond, const char* what) {
  if (!cond) std::printf("FAIL: %s\n", what);
  return cond;
}

template <typename T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
  std::unique_ptr<T[]> p(new T[v.size()]);
  for (size_t i = 0; i < v.size(); i++) p[i] = v[i];
  return p;
}

static Values make_values(const std::vector<size_t>& lengths) {
  Values out;
  for (size_t n : lengths) {
    Bytes b(n);
    for (auto& x : b) x = (uint8_t)(1 + rnd() % 255);
    out.push_back(b);
  }
  return out;
}

static Bytes stream_of(const Values& vals) {
  Bytes s;
  for (auto& v : vals) {
    uint32_t len = (uint32_t)v.size();
    const uint8_t* lp = (const uint8_t*)&len;
    s.insert(s.end(), lp, lp + 4);
    s.insert(s.end(), v.begin(), v.end());
  }
  return s;
}

static Bytes concat(const Values& vals) {
  Bytes s;
  for (auto& v : vals) s.insert(s.end(), v.begin(), v.end());
  return s;
}

// the walk on an exactly-sized copy; false when it throws
static bool walk(bool dict, const Bytes& stream, int64_t n,
                 std::vector<int64_t>* offs = nullptr, Bytes* stripped = nullptr) {
  auto in = exact(stream);
  std::vector<int64_t> o{0};
  Bytes by;
  int64_t total = 0;
  g_walks++;
  try {
    if (dict)
      lakesoul::str_walk_dict(in.get(), stream.size(), n, total, o, by);
    else
      lakesoul::str_walk_plain(in.get(), stream.size(), n, total, o);
  } catch (const std::exception&) {
    g_refused++;
    return false;
  }
  if (offs) *offs = o;
  if (stripped) *stripped = by;
  return true;
}

static bool check_valid(const char* name, const Values& vals) {
  Bytes stream = stream_of(vals), flat = concat(vals);
  bool ok = true;
  std::vector<int64_t> po, dofs;
  Bytes stripped;
  ok &= expect(walk(false, stream, (int64_t)vals.size(), &po), name);
  ok &= expect(walk(true, stream, (int64_t)vals.size(), &dofs, &stripped), name);
  ok &= expect(po == dofs && stripped == flat && po.back() == (int64_t)flat.size(), name);
  // prefix-strip twin, tables and stream exactly sized
  auto raw = exact(stream);
  auto off = exact(po);
  Bytes got = lsseg::strip_prefixes_host(raw.get(), (int64_t)stream.size(),
                                         off.get(), (int64_t)vals.size());
  ok &= expect(got == flat, name);
  // dictionary twin: every entry once, backwards, with a null row in front
  int64_t nent = (int64_t)vals.size();
  std::vector<int32_t> idx;
  for (int64_t k = nent - 1; k >= 0; k--) idx.push_back((int32_t)k);
  std::vector<uint8_t> valid((size_t)nent + 1, 1);
  valid[0] = 0;
  auto ip = exact(idx);
  auto vp = exact(valid);
  auto dp = exact(stripped);
  std::vector<int64_t> roffs;
  Bytes rbytes;
  int32_t st = lsseg::dict_strings_host(ip.get(), nent, off.get(), nent, dp.get(),
                                        (int64_t)stripped.size(), vp.get(),
                                        nent + 1, roffs, rbytes);
  Bytes want;
  for (int64_t k = nent - 1; k >= 0; k--)
    want.insert(want.end(), vals[(size_t)k].begin(), vals[(size_t)k].end());
  ok &= expect(st == 0 && rbytes == want && roffs[1] == 0, name);
  return ok;
}

int main() {
  bool ok = true;

  std::vector<size_t> phases;
  for (size_t i = 0; i < 18 * 18; i++) phases.push_back((i * 7 + i / 18) % 18);
  std::vector<size_t> empties{7};
  empties.insert(empties.end(), 5000, 0);
  empties.push_back(9);
  ok &= check_valid("phases", make_values(phases));
  ok &= check_valid("long", make_values({3, 70000, 5}));
  ok &= check_valid("empties", make_values(empties));
  ok &= check_valid("all empty", make_values(std::vector<size_t>(100, 0)));
  ok &= check_valid("none", {});

  // damaged streams, both walks
  Values three = make_values({3, 0, 5});
  Bytes good = stream_of(three);
  for (int dict = 0; dict < 2; dict++) {
    ok &= expect(walk(dict, good, 3), "valid stream");
    Bytes m = good;
    m.push_back(1);
    m.push_back(0);
    ok &= expect(!walk(dict, m, 4), "prefix past the end");
    m = stream_of(make_values({3}));
    const uint8_t nine[4] = {9, 0, 0, 0};
    m.insert(m.end(), nine, nine + 4);
    m.push_back('x');
    ok &= expect(!walk(dict, m, 2), "length past the end");
    m = stream_of(make_values({3}));
    m.insert(m.end(), 4, 0xFF);
    ok &= expect(!walk(dict, m, 2), "length of 4 GiB");
    ok &= expect(!walk(dict, good, 4), "one value too few");
    m = good;
    m.push_back('z');
    ok &= expect(!walk(dict, m, 3), "trailing bytes");
    ok &= expect(!walk(dict, good, 2), "one value too many");
    ok &= expect(!walk(dict, good, -1), "negative count");
    ok &= expect(walk(dict, {}, 0), "empty stream of no values");
    // a dictionary page shorter than its entry count, at every length
    Bytes big = stream_of(make_values(phases));
    for (size_t cut = 0; cut < big.size(); cut += (cut < 64 ? 1 : 37))
      ok &= expect(!walk(dict, Bytes(big.begin(), big.begin() + cut),
                         (int64_t)phases.size()), "truncated stream");
    for (size_t cut = 0; cut < good.size(); cut++)
      ok &= expect(!walk(dict, Bytes(good.begin(), good.begin() + cut), 3),
                   "truncated short stream");
  }

  // twins on tables that do not fit their buffers: nothing is read outside
  {
    Values vals = make_values({4, 9, 0, 17});
    Bytes stream = stream_of(vals), flat = concat(vals);
    std::vector<int64_t> off{0, 4, 13, 13, 30};
    // the raw stream cut short under valid offsets
    for (size_t cut = 0; cut < stream.size(); cut++) {
      Bytes s(stream.begin(), stream.begin() + cut);
      auto raw = exact(s);
      auto op = exact(off);
      Bytes got = lsseg::strip_prefixes_host(raw.get(), (int64_t)cut, op.get(), 4);
      ok &= expect(got.size() == 30, "cut raw stream: output size");
    }
    // dictionary: bad indices and a table that points past the bytes
    std::vector<int32_t> idx{0, 4, 2147483647, -1, 3, 1};
    auto ip = exact(idx);
    auto op = exact(off);
    auto dp = exact(flat);
    std::vector<int64_t> roffs;
    Bytes rbytes;
    int32_t st = lsseg::dict_strings_host(ip.get(), 6, op.get(), 4, dp.get(),
                                          (int64_t)flat.size(), nullptr, 6,
                                          roffs, rbytes);
    Bytes want = vals[0];
    want.insert(want.end(), vals[3].begin(), vals[3].end());
    want.insert(want.end(), vals[1].begin(), vals[1].end());
    ok &= expect(st != 0 && rbytes == want && roffs[2] == roffs[1] &&
                     roffs[3] == roffs[2] && roffs[4] == roffs[3],
                 "bad indices give empty rows and a status");
    // fewer indices than valid rows
    st = lsseg::dict_strings_host(ip.get(), 1, op.get(), 4, dp.get(),
                                  (int64_t)flat.size(), nullptr, 3, roffs, rbytes);
    ok &= expect(st != 0 && rbytes == vals[0], "rows without an index are empty");
    // dictionary bytes shorter than the offsets say
    Bytes shortd(flat.begin(), flat.begin() + 10);
    auto sp = exact(shortd);
    st = lsseg::dict_strings_host(ip.get(), 1, op.get(), 4, sp.get(), 10, nullptr, 1,
                                  roffs, rbytes);
    std::vector<int32_t> last{3};
    auto lp = exact(last);
    st = lsseg::dict_strings_host(lp.get(), 1, op.get(), 4, sp.get(), 10, nullptr, 1,
                                  roffs, rbytes);
    ok &= expect(rbytes.size() == 17 && rbytes[0] == 0,
                 "entry past the dictionary bytes reads as zeros");
  }

  std::printf("%s walks=%ld refused=%ld\n", ok ? "OK" : "FAIL", g_walks, g_refused);
  return ok ? 0 : 1;
}
