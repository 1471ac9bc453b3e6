// String predicates over an offsets + bytes column: compare against one
// literal, membership in a sorted set of literals, and LIKE. The per-row
// functions here are shared by the GPU kernel (csrc/hip/str_pred.hip) and
// its host twin at the end of this file, which the CPU filter route and the
// sanitizer program (tests/str_pred_san.cc) run.
//
// Values and literals are byte strings, ordered as unsigned bytes with a
// proper prefix first. A compiled operand is two flat arrays, `bytes`
// (uint8) and `meta` (int32):
//   one literal : bytes = the literal            meta = [len]
//   sorted set  : bytes = the literals in order  meta = [n, off[0] .. off[n]]
//   LIKE        : bytes = lit[T] then wild[T]    meta = [flags, nseg, T,
//                                                        off[0] .. off[nseg]]
// A LIKE pattern is cut at its unescaped '%' into non-empty segments;
// segment k is lit[off[k] .. off[k + 1]) and wild[j] != 0 marks a '_'.
// flags: 1 = the first segment starts the value, 2 = the last segment ends
// it, 4 = '_' is one UTF-8 code point (a byte, then every 10xxxxxx byte that
// follows) rather than one byte. Whatever the arrays hold, every read of
// them and of the column is clamped to its buffer.
#pragma once

#include <cstddef>
#include <cstdint>

#ifndef LSSEG_HD
#if defined(__HIPCC__) || defined(__HIP_DEVICE_COMPILE__)
#define LSSEG_HD __host__ __device__
#else
#define LSSEG_HD
#endif
#endif

namespace lspred {

enum Op : int {
  OP_EQ = 0, OP_NOTEQ = 1, OP_LT = 2, OP_LTEQ = 3, OP_GT = 4, OP_GTEQ = 5,
  OP_IN = 6, OP_LIKE = 7, OP_NOT_LIKE = 8, OP_COUNT = 9
};
enum LikeFlags : int { LIKE_START = 1, LIKE_END = 2, LIKE_UTF8 = 4 };

struct Operand {
  const uint8_t* bytes;
  int64_t nbytes;
  const int32_t* meta;
  int64_t nmeta;
};

// least meta length of a well-formed operand of `op`
LSSEG_HD inline int64_t min_meta(int op) {
  return op == OP_IN ? 2 : op >= OP_LIKE ? 4 : 1;
}

LSSEG_HD inline int64_t clampi(int64_t x, int64_t lo, int64_t hi) {
  return x < lo ? lo : x > hi ? hi : x;
}

LSSEG_HD inline bool is_cont(uint8_t b) { return (b & 0xC0) == 0x80; }

// -1, 0, +1. Dwords where a and b sit at the same phase of their words,
// bytes at the edges and otherwise.
LSSEG_HD inline int compare(const uint8_t* a, int64_t alen, const uint8_t* b,
                            int64_t blen) {
  int64_t n = alen < blen ? alen : blen, i = 0;
  if (n >= 8 && (((uintptr_t)a ^ (uintptr_t)b) & 3) == 0) {
    for (; ((uintptr_t)(a + i) & 3) != 0; i++)
      if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    for (; i + 4 <= n; i += 4) {
      uint32_t x, y;
      __builtin_memcpy(&x, __builtin_assume_aligned(a + i, 4), 4);
      __builtin_memcpy(&y, __builtin_assume_aligned(b + i, 4), 4);
      if (x != y) {
        x = __builtin_bswap32(x);
        y = __builtin_bswap32(y);
        return x < y ? -1 : 1;
      }
    }
  }
  for (; i < n; i++)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return alen == blen ? 0 : alen < blen ? -1 : 1;
}

struct SeqCompare {
  LSSEG_HD int operator()(const uint8_t* a, int64_t alen, const uint8_t* b,
                          int64_t blen) const {
    return compare(a, alen, b, blen);
  }
};

LSSEG_HD inline bool cmp_holds(int op, int c) {
  switch (op) {
    case OP_EQ: return c == 0;
    case OP_NOTEQ: return c != 0;
    case OP_LT: return c < 0;
    case OP_LTEQ: return c <= 0;
    case OP_GT: return c > 0;
    default: return c >= 0;
  }
}

// segment [pos ...) of the value against lit/wild, reading below hi only:
// the end of the match, -1 when there is none
LSSEG_HD inline int64_t seg_fwd(const uint8_t* v, int64_t pos, int64_t hi,
                                const uint8_t* lit, const uint8_t* wild,
                                int64_t slen, bool utf8) {
  int64_t p = pos;
  for (int64_t j = 0; j < slen; j++) {
    if (p >= hi) return -1;
    if (wild[j]) {
      p++;
      if (utf8)
        while (p < hi && is_cont(v[p])) p++;
    } else {
      if (v[p] != lit[j]) return -1;
      p++;
    }
  }
  return p;
}

// the segment backwards from `end`, reading at or above lo only: the start
// of the match, -1 when there is none
LSSEG_HD inline int64_t seg_bwd(const uint8_t* v, int64_t lo, int64_t end,
                                const uint8_t* lit, const uint8_t* wild,
                                int64_t slen, bool utf8) {
  int64_t p = end;
  for (int64_t j = slen - 1; j >= 0; j--) {
    if (p <= lo) return -1;
    p--;
    if (wild[j]) {
      if (utf8)
        while (p > lo && is_cont(v[p])) p--;
    } else if (v[p] != lit[j]) {
      return -1;
    }
  }
  return p;
}

// may a match of a middle segment start at pos?
LSSEG_HD inline bool like_candidate(const uint8_t* v, int64_t pos, bool utf8) {
  return !utf8 || !is_cont(v[pos]);
}

// leftmost match of a middle segment inside [lo, hi): its end, or -1
struct SeqFind {
  LSSEG_HD int64_t operator()(const uint8_t* v, int64_t lo, int64_t hi,
                              const uint8_t* lit, const uint8_t* wild,
                              int64_t slen, bool utf8) const {
    for (int64_t pos = lo; pos + slen <= hi; pos++) {
      if (!like_candidate(v, pos, utf8)) continue;
      int64_t e = seg_fwd(v, pos, hi, lit, wild, slen, utf8);
      if (e >= 0) return e;
    }
    return -1;
  }
};

template <class Find>
LSSEG_HD inline bool like_match(const Operand& o, const uint8_t* v, int64_t n,
                                Find find) {
  if (o.nmeta < 4) return false;
  int flags = o.meta[0];
  int64_t nseg = clampi(o.meta[1], 0, o.nmeta - 4);
  int64_t half = o.nbytes >> 1;
  bool as = flags & LIKE_START, ae = flags & LIKE_END, utf8 = flags & LIKE_UTF8;
  if (nseg == 0) return (as && ae) ? n == 0 : true;
  const uint8_t* lit = o.bytes;
  const uint8_t* wild = o.bytes + half;
  const int32_t* off = o.meta + 3;
  int64_t lo = 0, hi = n, k0 = 0, k1 = nseg;
  if (ae) {
    int64_t s = clampi(off[nseg - 1], 0, half), e = clampi(off[nseg], s, half);
    if (as && nseg == 1)
      return seg_fwd(v, 0, n, lit + s, wild + s, e - s, utf8) == n;
    hi = seg_bwd(v, 0, n, lit + s, wild + s, e - s, utf8);
    if (hi < 0) return false;
    k1--;
  }
  if (as) {
    int64_t s = clampi(off[0], 0, half), e = clampi(off[1], s, half);
    lo = seg_fwd(v, 0, hi, lit + s, wild + s, e - s, utf8);
    if (lo < 0) return false;
    k0++;
  }
  for (int64_t k = k0; k < k1; k++) {
    int64_t s = clampi(off[k], 0, half), e = clampi(off[k + 1], s, half);
    if (e == s) continue;  // only a damaged program has an empty segment
    lo = find(v, lo, hi, lit + s, wild + s, e - s, utf8);
    if (lo < 0) return false;
  }
  return true;
}

template <class Cmp>
LSSEG_HD inline bool set_contains(const Operand& o, const uint8_t* v, int64_t n,
                                  Cmp cmp) {
  if (o.nmeta < 2) return false;
  int64_t nlit = clampi(o.meta[0], 0, o.nmeta - 2);
  const int32_t* off = o.meta + 1;
  int64_t lo = 0, hi = nlit;
  while (lo < hi) {
    int64_t mid = lo + ((hi - lo) >> 1);
    int64_t s = clampi(off[mid], 0, o.nbytes), e = clampi(off[mid + 1], s, o.nbytes);
    int c = cmp(v, n, o.bytes + s, e - s);
    if (c == 0) return true;
    if (c < 0) hi = mid;
    else lo = mid + 1;
  }
  return false;
}

// the predicate on one value (the caller has dealt with a null row)
template <class Cmp, class Find>
LSSEG_HD inline bool row_pred(int op, const Operand& o, const uint8_t* v,
                              int64_t n, Cmp cmp, Find find) {
  if (op == OP_IN) return set_contains(o, v, n, cmp);
  if (op == OP_LIKE || op == OP_NOT_LIKE)
    return like_match(o, v, n, find) != (op == OP_NOT_LIKE);
  if (o.nmeta < 1) return false;
  int64_t llen = clampi(o.meta[0], 0, o.nbytes);
  if (op == OP_EQ || op == OP_NOTEQ) {
    if (n != llen) return op == OP_NOTEQ;
  }
  return cmp_holds(op, cmp(v, n, o.bytes, llen));
}

// row i of the column: its bytes start at bytes + s and there are n of
// them; a damaged table cannot point outside [0, nbytes]
template <typename OffT>
LSSEG_HD inline void row_range(const OffT* offsets, int64_t i, int64_t nbytes,
                               int64_t& s, int64_t& n) {
  s = clampi((int64_t)offsets[i], 0, nbytes);
  n = clampi((int64_t)offsets[i + 1], s, nbytes) - s;
}

}  // namespace lspred

#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <string>
#include <vector>

namespace lspred {

// one literal
inline void compile_literal(const uint8_t* lit, int64_t len,
                            std::vector<uint8_t>& bytes,
                            std::vector<int32_t>& meta) {
  bytes.assign(lit, lit + (len > 0 ? len : 0));
  meta.assign(1, (int32_t)bytes.size());
}

// a set of literals: sorted in byte order, duplicates dropped
inline void compile_set(std::vector<std::string> lits,
                        std::vector<uint8_t>& bytes,
                        std::vector<int32_t>& meta) {
  std::sort(lits.begin(), lits.end(), [](const std::string& a, const std::string& b) {
    return compare((const uint8_t*)a.data(), (int64_t)a.size(),
                   (const uint8_t*)b.data(), (int64_t)b.size()) < 0;
  });
  lits.erase(std::unique(lits.begin(), lits.end()), lits.end());
  bytes.clear();
  meta.assign(1, (int32_t)lits.size());
  meta.push_back(0);
  for (const auto& s : lits) {
    bytes.insert(bytes.end(), s.begin(), s.end());
    meta.push_back((int32_t)bytes.size());
  }
}

// a LIKE pattern; escape < 0: no escape character. The escape character
// makes the byte after it literal; as the pattern's last byte it stands for
// itself.
inline void compile_like(const uint8_t* pat, int64_t plen, int escape,
                         bool utf8, std::vector<uint8_t>& bytes,
                         std::vector<int32_t>& meta) {
  std::vector<uint8_t> lit, wild;
  std::vector<int32_t> off(1, 0);
  bool any = false, start = true, last_pct = false;
  for (int64_t i = 0; i < plen; i++) {
    uint8_t c = pat[i];
    if (escape >= 0 && c == (uint8_t)escape) {
      if (i + 1 < plen) c = pat[++i];
      lit.push_back(c);
      wild.push_back(0);
      last_pct = false;
    } else if (c == '%') {
      if (!any) start = false;
      if ((int32_t)lit.size() > off.back()) off.push_back((int32_t)lit.size());
      last_pct = true;
    } else {
      lit.push_back(c == '_' ? 0 : c);
      wild.push_back(c == '_' ? 1 : 0);
      last_pct = false;
    }
    any = true;
  }
  if ((int32_t)lit.size() > off.back()) off.push_back((int32_t)lit.size());
  int32_t flags = (start ? LIKE_START : 0) | (!last_pct ? LIKE_END : 0) |
                  (utf8 ? LIKE_UTF8 : 0);
  bytes = lit;
  bytes.insert(bytes.end(), wild.begin(), wild.end());
  meta.assign({flags, (int32_t)off.size() - 1, (int32_t)lit.size()});
  meta.insert(meta.end(), off.begin(), off.end());
}

// Host twin of the kernel: out[i] = validity[i] && pred(row i)
template <typename OffT>
inline void str_pred_mask_host(const OffT* offsets, int64_t nrows,
                               const uint8_t* bytes, int64_t nbytes,
                               const uint8_t* validity, int op, const Operand& o,
                               uint8_t* out) {
  for (int64_t i = 0; i < nrows; i++) {
    if (validity && !validity[i]) {
      out[i] = 0;
      continue;
    }
    int64_t s, n;
    row_range(offsets, i, nbytes, s, n);
    out[i] = row_pred(op, o, bytes + s, n, SeqCompare(), SeqFind()) ? 1 : 0;
  }
}

}  // namespace lspred
#endif
