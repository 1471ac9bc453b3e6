// Bounds check of the string predicates' shared code (csrc/cpp/str_pred.h):
// the pattern / set compilers and the per-row matcher that the GPU kernel
// (csrc/hip/str_pred.hip) also runs — built with
// -fsanitize=address,undefined by
// tests/test_str_pred.py::test_str_pred_sanitizer_clean. The column, the
// operand and the mask each sit in an exactly-sized heap buffer, so any read
// or write past either end is a sanitizer report.
// - Random patterns over a small alphabet ('%', '_', the escape character,
//   letters, a two-byte code point) against random values, binary and UTF-8:
//   the mask equals a backtracking matcher written here.
// - Patterns that end in the escape character, values cut in the middle of a
//   code point, lone continuation bytes: run for memory safety.
// - Compare and IN over values at every phase of a word, int32 and int64
//   offsets, a slice with a non-zero base: equal to memcmp order.
// - Damaged offsets (negative, past the bytes, decreasing, INT32_MAX) and
//   damaged operands (segment offsets / set offsets / counts outside their
//   arrays): read nothing outside.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../str_pred.h"

using Bytes = std::vector<uint8_t>;

static long g_rows = 0;
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

// the mask of one predicate over `vals`, everything on exact heap buffers;
// OffT offsets, `base` junk bytes in front of the first row
template <typename OffT>
static std::vector<uint8_t> run(const std::vector<Bytes>& vals, int op,
                                const Bytes& ob, const std::vector<int32_t>& om,
                                int64_t base = 0, const uint8_t* validity = nullptr) {
  Bytes blob((size_t)base, 0x5A);
  std::vector<OffT> offs(1, (OffT)base);
  for (auto& v : vals) {
    blob.insert(blob.end(), v.begin(), v.end());
    offs.push_back((OffT)blob.size());
  }
  auto pb = exact(blob);
  auto po = exact(offs);
  auto pob = exact(ob);
  auto pom = exact(om);
  std::unique_ptr<uint8_t[]> out(new uint8_t[vals.size()]);
  lspred::Operand o{pob.get(), (int64_t)ob.size(), pom.get(), (int64_t)om.size()};
  lspred::str_pred_mask_host(po.get(), (int64_t)vals.size(), pb.get(),
                             (int64_t)blob.size(), validity, op, o, out.get());
  g_rows += (long)vals.size();
  return std::vector<uint8_t>(out.get(), out.get() + vals.size());
}

// ---- reference LIKE: tokens + backtracking ----------------------------- //

struct Tok { int kind; uint8_t b; };  // 0 literal, 1 '_', 2 '%'

static std::vector<Tok> tokens(const Bytes& pat, int escape) {
  std::vector<Tok> t;
  for (size_t i = 0; i < pat.size(); i++) {
    uint8_t c = pat[i];
    if (escape >= 0 && c == (uint8_t)escape) {
      if (i + 1 < pat.size()) c = pat[++i];
      t.push_back({0, c});
    } else if (c == '%') t.push_back({2, 0});
    else if (c == '_') t.push_back({1, 0});
    else t.push_back({0, c});
  }
  return t;
}

static bool ref_like(const std::vector<Tok>& t, size_t ti, const Bytes& v,
                     size_t vi, bool utf8) {
  if (ti == t.size()) return vi == v.size();
  if (t[ti].kind == 2) {
    for (size_t k = vi; k <= v.size(); k++) {
      // a '%' run may end anywhere for binary; for valid UTF-8 values ending
      // inside a code point never leads to a match of what follows unless
      // nothing follows, which k == size covers
      if (ref_like(t, ti + 1, v, k, utf8)) return true;
    }
    return false;
  }
  if (vi >= v.size()) return false;
  if (t[ti].kind == 1) {
    if (utf8 && lspred::is_cont(v[vi])) return false;
    size_t k = vi + 1;
    if (utf8)
      while (k < v.size() && lspred::is_cont(v[k])) k++;
    return ref_like(t, ti + 1, v, k, utf8);
  }
  return v[vi] == t[ti].b && ref_like(t, ti + 1, v, vi + 1, utf8);
}

static Bytes random_value(bool utf8, int maxlen) {
  Bytes v;
  int n = (int)(rnd() % (uint32_t)(maxlen + 1));
  while ((int)v.size() < n) {
    uint32_t r = rnd() % 8;
    if (r == 0) {
      if (utf8) { v.push_back(0xC3); v.push_back(0xA9); }
      else v.push_back(0xA9);
    } else if (r == 1) v.push_back('%');
    else if (r == 2) v.push_back('_');
    else if (r == 3) v.push_back('\\');
    else v.push_back((uint8_t)('a' + r % 2));
  }
  return v;
}

static Bytes random_pattern(bool utf8) {
  Bytes p;
  int n = (int)(rnd() % 7);
  for (int i = 0; i < n; i++) {
    uint32_t r = rnd() % 10;
    if (r < 3) p.push_back('%');
    else if (r < 5) p.push_back('_');
    else if (r == 5) p.push_back('\\');
    else if (r == 6 && utf8) { p.push_back(0xC3); p.push_back(0xA9); }
    else p.push_back((uint8_t)('a' + r % 2));
  }
  return p;
}

static bool like_matches_reference() {
  bool ok = true;
  for (int utf8 = 0; utf8 <= 1; utf8++) {
    std::vector<Bytes> vals;
    for (int i = 0; i < 300; i++) vals.push_back(random_value(utf8, 9));
    for (int it = 0; it < 600 && ok; it++) {
      Bytes pat = random_pattern(utf8);
      Bytes ob;
      std::vector<int32_t> om;
      lspred::compile_like(pat.data(), (int64_t)pat.size(), '\\', utf8, ob, om);
      auto m32 = run<int32_t>(vals, lspred::OP_LIKE, ob, om);
      auto m64 = run<int64_t>(vals, lspred::OP_NOT_LIKE, ob, om, 13);
      auto t = tokens(pat, '\\');
      for (size_t i = 0; i < vals.size(); i++) {
        bool want = ref_like(t, 0, vals[i], 0, utf8);
        if (m32[i] != (want ? 1 : 0) || m64[i] != (want ? 0 : 1)) {
          std::printf("FAIL: like utf8=%d pattern '%.*s' value '%.*s' want %d\n",
                      utf8, (int)pat.size(), (const char*)pat.data(),
                      (int)vals[i].size(), (const char*)vals[i].data(), (int)want);
          ok = false;
          break;
        }
      }
    }
  }
  return ok;
}

// memory safety only: invalid UTF-8 in value and pattern, trailing escapes
static bool like_on_broken_text() {
  std::vector<Bytes> vals = {
      {}, {0xC3}, {'a', 0xC3}, {0xA9}, {0xA9, 0xA9, 0xA9}, {'a', 0xE2, 0x82},
      {0xE2, 0x82, 0xAC, 0xE2}, {0xF0, 0x9F}, {0x80, 'a', 0x80}, {0xFF, 0xFF},
      {'a', 'b', 0xC3}, {0xC3, 0xC3, 0xA9, 0xA9}};
  std::vector<Bytes> pats = {
      {'\\'}, {'a', '\\'}, {'%', '\\'}, {'_', '\\'}, {'\\', '\\', '\\'}, {'_'},
      {'_', '_'}, {'%', '_'}, {'_', '%'}, {'%', '_', '%'}, {0xC3}, {'%', 0xA9},
      {'_', 0xA9, '%'}, {'%', 0xC3, '_'}, {'a', '_', 0xC3}, {'%', '_', '_', '_'}};
  for (int utf8 = 0; utf8 <= 1; utf8++)
    for (int esc : {-1, (int)'\\', (int)'_', (int)'%'})
      for (auto& p : pats) {
        Bytes ob;
        std::vector<int32_t> om;
        lspred::compile_like(p.data(), (int64_t)p.size(), esc, utf8, ob, om);
        run<int32_t>(vals, lspred::OP_LIKE, ob, om);
        run<int64_t>(vals, lspred::OP_NOT_LIKE, ob, om, 5);
      }
  // a pattern that ends in the escape character: the escape stands for itself
  Bytes ob;
  std::vector<int32_t> om;
  const uint8_t p[] = {'a', '\\'};
  lspred::compile_like(p, 2, '\\', true, ob, om);
  auto m = run<int32_t>({{'a', '\\'}, {'a'}, {'a', '\\', '\\'}}, lspred::OP_LIKE, ob, om);
  return expect(m[0] == 1 && m[1] == 0 && m[2] == 0, "trailing escape is a literal");
}

static int mem_order(const Bytes& a, const Bytes& b) {
  size_t n = a.size() < b.size() ? a.size() : b.size();
  int c = n ? std::memcmp(a.data(), b.data(), n) : 0;
  if (c) return c < 0 ? -1 : 1;
  return a.size() == b.size() ? 0 : a.size() < b.size() ? -1 : 1;
}

static bool compare_and_in() {
  bool ok = true;
  std::vector<size_t> lens = {0, 1, 3, 4, 7, 8, 9, 15, 16, 17, 63, 64, 65, 257};
  for (size_t ll : {0, 1, 4, 8, 9, 65}) {
    Bytes lit(ll);
    for (auto& x : lit) x = (uint8_t)(rnd() % 3 == 0 ? 0xFF : rnd() % 256);
    std::vector<Bytes> vals;
    for (size_t n : lens)
      for (int ph = 0; ph < 8; ph++) {
        vals.push_back(Bytes((size_t)ph, 0x70));  // shifts the next value's phase
        Bytes v(n);
        for (size_t i = 0; i < n; i++) v[i] = i < ll ? lit[i] : (uint8_t)rnd();
        if (n && ph % 3 == 1) v[n - 1] ^= 0x80;
        if (n && ph % 3 == 2) v[0] ^= 0x01;
        vals.push_back(v);
      }
    vals.push_back(lit);
    Bytes ob;
    std::vector<int32_t> om;
    lspred::compile_literal(lit.data(), (int64_t)lit.size(), ob, om);
    for (int op = lspred::OP_EQ; op <= lspred::OP_GTEQ; op++) {
      auto a = run<int32_t>(vals, op, ob, om);
      auto b = run<int64_t>(vals, op, ob, om, 3);
      for (size_t i = 0; i < vals.size(); i++) {
        bool want = lspred::cmp_holds(op, mem_order(vals[i], lit));
        ok &= expect(a[i] == (want ? 1 : 0) && b[i] == a[i], "compare equals memcmp order");
      }
    }
    // IN: the literal, some of the values, duplicates, the empty string
    std::vector<std::string> set = {std::string(lit.begin(), lit.end()), "", "abc", "abc"};
    for (size_t i = 0; i < vals.size(); i += 5)
      set.push_back(std::string(vals[i].begin(), vals[i].end()));
    lspred::compile_set(set, ob, om);
    auto a = run<int32_t>(vals, lspred::OP_IN, ob, om, 7);
    for (size_t i = 0; i < vals.size(); i++) {
      bool want = false;
      for (auto& s : set) want |= s == std::string(vals[i].begin(), vals[i].end());
      ok &= expect(a[i] == (want ? 1 : 0), "IN equals a linear search");
    }
  }
  Bytes ob;
  std::vector<int32_t> om;
  lspred::compile_set({}, ob, om);
  auto m = run<int32_t>({{}, {'a'}}, lspred::OP_IN, ob, om);
  ok &= expect(m[0] == 0 && m[1] == 0, "the empty set matches nothing");
  return ok;
}

// tables that do not fit their buffers: nothing is read outside
static bool damaged_tables() {
  Bytes blob(40);
  for (auto& x : blob) x = (uint8_t)('a' + rnd() % 3);
  std::vector<std::vector<int64_t>> tables = {
      {0, 50, 60}, {-5, 10, 20}, {30, 10, 45}, {0, INT32_MAX, 3}, {39, 41, 40},
      {-7, -3, -1}, {100, 200, 300}, {0, 40, 41}};
  std::vector<std::pair<Bytes, std::vector<int32_t>>> operands;
  std::vector<int> ops;
  auto add = [&](int op, Bytes b, std::vector<int32_t> m) {
    ops.push_back(op);
    operands.push_back({b, m});
  };
  Bytes ob;
  std::vector<int32_t> om;
  const uint8_t pat[] = {'a', '%', 'b', '_', '%', 'c'};
  lspred::compile_like(pat, 6, '\\', true, ob, om);
  add(lspred::OP_LIKE, ob, om);
  for (size_t k = 0; k < om.size(); k++) {  // every meta word damaged in turn
    for (int32_t bad : {-1, 1000, INT32_MAX, INT32_MIN}) {
      auto m = om;
      m[k] = bad;
      add(lspred::OP_LIKE, ob, m);
    }
  }
  add(lspred::OP_LIKE, {}, om);              // no bytes at all
  add(lspred::OP_LIKE, ob, {7, 3, 2, 0});    // fewer offsets than segments
  lspred::compile_set({"a", "ab", "b", "abc"}, ob, om);
  add(lspred::OP_IN, ob, om);
  for (size_t k = 0; k < om.size(); k++)
    for (int32_t bad : {-1, 1000, INT32_MAX}) {
      auto m = om;
      m[k] = bad;
      add(lspred::OP_IN, ob, m);
    }
  add(lspred::OP_EQ, {'a', 'b'}, {50});
  add(lspred::OP_LT, {'a', 'b'}, {-4});
  add(lspred::OP_GTEQ, {}, {3});
  auto pb = exact(blob);
  for (auto& t : tables) {
    std::vector<int32_t> t32;
    for (auto x : t) t32.push_back((int32_t)x);
    auto p64 = exact(t);
    auto p32 = exact(t32);
    for (size_t i = 0; i < ops.size(); i++) {
      auto pob = exact(operands[i].first);
      auto pom = exact(operands[i].second);
      lspred::Operand o{pob.get(), (int64_t)operands[i].first.size(), pom.get(),
                        (int64_t)operands[i].second.size()};
      if (o.nmeta < lspred::min_meta(ops[i])) continue;  // the bindings refuse these
      uint8_t out[2];
      lspred::str_pred_mask_host(p64.get(), 2, pb.get(), (int64_t)blob.size(),
                                 nullptr, ops[i], o, out);
      lspred::str_pred_mask_host(p32.get(), 2, pb.get(), (int64_t)blob.size(),
                                 nullptr, ops[i], o, out);
      g_rows += 4;
    }
  }
  return true;
}

int main() {
  bool ok = true;
  ok &= like_matches_reference();
  ok &= like_on_broken_text();
  ok &= compare_and_in();
  ok &= damaged_tables();
  std::printf("%s: %ld rows\n", ok ? "OK" : "FAILED", g_rows);
  return ok ? 0 : 1;
}
