// Walks of length-prefixed byte-array streams for the GPU string route
// (read_unit.h, UD_STR): the host reads the u32 prefixes only and never
// touches the payload. Plain functions on (pointer, length) so that the
// sanitizer program (tests/str_walk_san.cc) runs them without a file.
// Every prefix and every length is checked against the end of the stream
// before it is used; a stream with fewer or more values than announced, or
// with bytes left over, throws.
#pragma once

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

namespace lakesoul {

// PLAIN (u32 len, bytes)* stream of exactly `expect` values in [p, p + n).
// Appends one end offset per value to `offs` (exclusive running sum of the
// lengths, continued from `running`, which is updated): with a leading 0
// they are the dense offsets of the column.
inline void str_walk_plain(const uint8_t* p, size_t n, int64_t expect,
                           int64_t& running, std::vector<int64_t>& offs) {
  if (expect < 0) throw std::runtime_error("string walk: negative value count");
  size_t pos = 0;
  for (int64_t i = 0; i < expect; i++) {
    if (n - pos < 4)
      throw std::runtime_error("string walk: length prefix past the end");
    uint32_t len;
    std::memcpy(&len, p + pos, 4);
    pos += 4;
    if ((size_t)len > n - pos)
      throw std::runtime_error("string walk: value past the end");
    pos += (size_t)len;
    running += (int64_t)len;
    offs.push_back(running);
  }
  if (pos != n)
    throw std::runtime_error("string walk: bytes left after the last value");
}

// Dictionary page of exactly `nent` entries: the same walk, and the entry
// bytes, stripped of their prefixes, appended to `bytes`.
inline void str_walk_dict(const uint8_t* p, size_t n, int64_t nent,
                          int64_t& running, std::vector<int64_t>& offs,
                          std::vector<uint8_t>& bytes) {
  if (nent < 0) throw std::runtime_error("string walk: negative entry count");
  size_t pos = 0;
  for (int64_t i = 0; i < nent; i++) {
    if (n - pos < 4)
      throw std::runtime_error("dictionary page shorter than its entry count");
    uint32_t len;
    std::memcpy(&len, p + pos, 4);
    pos += 4;
    if ((size_t)len > n - pos)
      throw std::runtime_error("dictionary page: entry past the end");
    bytes.insert(bytes.end(), p + pos, p + pos + len);
    pos += (size_t)len;
    running += (int64_t)len;
    offs.push_back(running);
  }
  if (pos != n)
    throw std::runtime_error("dictionary page: bytes left after the last entry");
}

}  // namespace lakesoul
