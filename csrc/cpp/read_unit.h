// Unit reader: read ALL files of one scan unit (bucket) in one call.
//
// Two-stage design so the python binding can allocate pinned torch
// tensors and have chunk payloads land in them directly (no second
// copy):
//   stage1: open files (via a footer/mmap cache — the analog of the
//           reference's file-meta cache, session.rs:86-105), decompress
//           every (file, column, row-group) chunk across the persistent
//           thread pool, compute the buffer layout and RLE run table.
//   fill:   parallel memcpy of chunk payloads straight into the caller's
//           destination buffers.
//
// Buffer layout (8-byte aligned so torch dtype views work):
//   values  : per-(file,col) dense PLAIN payloads, row-group chunks
//             contiguous (a no-null column is ONE device view);
//             dict-index payloads (+8 pad); string bytes
//   validity: per-(file,col) validity bytes, contiguous across RGs
//   dicts   : concatenated per-RG dictionaries (element bias applied in
//             the GPU expansion kernel)
//   runs    : int64 [m][6] {dense_out_off, n, is_literal,
//             value_or_abs_bitoff, bit_width, dict_elem_bias}
//   soffs   : int64 string offsets per (file,col), rebased across chunks
//   enc     : int64 [m][6], GPU-decoded DELTA_BINARY_PACKED /
//             BYTE_STREAM_SPLIT columns (gpu_delta; UD_ENC != 0). Their raw
//             page payloads sit in values like dict-index payloads: each
//             page 8-byte aligned, each chunk padded to 8, the region +8.
//             Per (file,col): its page rows, then its miniblock rows.
//               delta page : {dense_out_off, n, first_value,
//                             first miniblock (index among the column's
//                             miniblock rows), 0, 0}
//               miniblock  : {dense_out_off of the first value it
//                             produces, n, abs_bit_off into values,
//                             bit_width, min_delta, page row}
//               split page : {dense_out_off, n, abs_byte_off into values,
//                             0, 0, 0}
//             dense offsets count stored (non-null) values across the
//             column's chunks. Every row comes from delta_walk (delta.h):
//             its span is validated against the page before it is listed.
//
// GPU string route (gpu_strings; UD_STR != 0, chosen per (file, column)):
// the host reads length prefixes only and the GPU moves the bytes
// (csrc/hip/strings.hip). The decoded column is the same (offsets, compact
// bytes, validity) triple as on the host route. A column takes a kind only
// when every chunk of it in the file is of that kind; mixed columns, lists
// and nested leaves stay host-assembled (UD_STR = 0).
//   UD_STR_PLAIN: values holds the chunks' decompressed PLAIN streams
//             (u32 len, bytes)* back to back, unpadded, at UD_VAL_OFF /
//             UD_VAL_LEN. soffs holds the DENSE offsets (UD_DENSE_N + 1
//             entries from 0: running sum of the lengths of the stored,
//             non-null values), so dense value i sits at
//             val_off + doff[i] + 4 * (i + 1). UD_SBYTES_LEN is the compact
//             byte total, UD_SBYTES_OFF = -1.
//   UD_STR_DICT: values and runs hold the RLE index pages as for a
//             fixed-width dictionary column (run bias = entries of the
//             column's earlier chunks). dicts holds the entry bytes of all
//             chunks stripped of their prefixes (UD_DICT_OFF / UD_DICT_LEN),
//             soffs one table of entry offsets (entries + 1, from 0;
//             entries = UD_SBYTES_LEN, UD_SBYTES_OFF = -1). RLE run values
//             are checked against the chunk's dictionary here; bit-packed
//             indices are checked by the kernel.
#pragma once

#include <atomic>
#include <cstring>
#include <list>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include <chrono>

#include "delta.h"
#include "parquet_file.h"
#include "rle.h"
#include "str_walk.h"
#include "thread_pool.h"
#include "unit_desc.h"

namespace lakesoul {

// ---------------------------------------------------------------------- //
// file handle cache (footer + mmap reuse across scans/steps)
// ---------------------------------------------------------------------- //

class FileCache {
 public:
  static FileCache& instance() {
    static FileCache* c = new FileCache();
    return *c;
  }

  std::shared_ptr<ParquetFile> open(const std::string& path) {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = map_.find(path);
    if (it != map_.end()) {
      lru_.splice(lru_.begin(), lru_, it->second.second);
      return it->second.first;
    }
    auto f = std::make_shared<ParquetFile>(path);
    lru_.push_front(path);
    map_[path] = {f, lru_.begin()};
    while (map_.size() > capacity_) {
      map_.erase(lru_.back());
      lru_.pop_back();
    }
    return f;
  }

  void invalidate(const std::string& path) {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = map_.find(path);
    if (it != map_.end()) {
      lru_.erase(it->second.second);
      map_.erase(it);
    }
  }

 private:
  std::mutex mu_;
  size_t capacity_ = 512;
  std::list<std::string> lru_;
  std::unordered_map<
      std::string,
      std::pair<std::shared_ptr<ParquetFile>, std::list<std::string>::iterator>>
      map_;
};

// ---------------------------------------------------------------------- //

struct UnitColumn {
  int file_idx;
  std::string name;
  bool present = false;
  bool is_string = false;
  bool is_dict = false;
  int physical = 0;
  int64_t num_values = 0;
  int64_t null_count = 0;
  int64_t val_off = 0, val_len = 0;
  int64_t validity_off = -1;
  int64_t dict_off = 0, dict_len = 0;
  int64_t run_off = 0, run_cnt = 0;
  int64_t dense_n = 0;
  int32_t enc = 0;  // ParquetFile::EncKind: raw pages, decoded on the GPU
  int64_t enc_off = 0, enc_cnt = 0, enc_pages = 0;  // rows of UnitStage::enc
  int64_t soff_off = -1;
  int64_t sbytes_off = 0, sbytes_len = 0;
  int32_t str_kind = UD_STR_HOST;  // GPU string route, see the layout comment
  bool is_list = false;  // element values in the sbytes region, element
                         // offsets in soffs, ROW validity in validity
};

inline int64_t ru_align8(int64_t x) { return (x + 7) & ~7LL; }

struct UnitStage {
  struct FileData {
    std::shared_ptr<ParquetFile> f;
    std::vector<std::vector<ParquetFile::ChunkData>> chunks;
    std::vector<int> col_idx;
  };
  struct StrDecoded {
    std::vector<int64_t> offs;
    std::vector<uint8_t> bytes;
    std::vector<uint8_t> row_valid;  // lists: per-row validity (may be empty)
  };

  int64_t t_open_us = 0, t_chunks_us = 0, t_layout_us = 0;
  size_t ncols = 0;
  std::vector<FileData> files;
  std::vector<UnitColumn> cols;
  std::vector<int64_t> file_rows;
  std::vector<int64_t> runs;  // [m][6]
  std::vector<int64_t> enc;   // [m][6], see the layout comment
  std::vector<int64_t> snappy_jobs;  // [m][4]: comp_off, comp_len, dst_off(values), dst_len
  std::vector<int64_t> zstd_jobs;    // [m][4]: same layout, zstd frames
  struct HostJob {
    int file_idx;
    int64_t file_off, comp_len, dst_off, dst_len;
    int32_t codec;
  };
  std::vector<HostJob> host_jobs;
  // Huffman-only zstd pages, decoded by zstd_huf.hip: jobs as zstd_jobs;
  // huf_src[i] is where fill copies job i's frame from (HostJob with
  // dst_off = its place in comp)
  std::vector<int64_t> huf_jobs;
  std::vector<HostJob> huf_src;
  // LZ4_RAW pages, decoded by lz4.hip: jobs as snappy_jobs; lz4_src as
  // huf_src (the two share the tail of comp)
  std::vector<int64_t> lz4_jobs;
  std::vector<HostJob> lz4_src;
  // GZIP pages, decoded by gzip.hip: as lz4_jobs and lz4_src (all three
  // share the tail of comp)
  std::vector<int64_t> gzip_jobs;
  std::vector<HostJob> gzip_src;
  std::vector<std::unique_ptr<StrDecoded>> str_cols;
  int64_t values_size = 0, validity_size = 0, dicts_size = 0, soffs_size = 0,
          comp_size = 0;
};

inline std::unique_ptr<UnitStage> read_unit_stage1(
    const std::vector<std::string>& paths, const std::vector<std::string>& names,
    bool gpu_snappy = false, bool gpu_zstd = false,
    double gpu_zstd_frac = 1.0, bool gpu_delta = false, bool gpu_huf = false,
    bool gpu_lz4 = false, bool gpu_strings = false, bool gpu_gzip = false) {
  auto st = std::make_unique<UnitStage>();
  UnitStage& S = *st;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto us = [](auto a, auto b) {
    return std::chrono::duration_cast<std::chrono::microseconds>(b - a).count();
  };
  auto tp0 = now();
  size_t nfiles = paths.size();
  S.ncols = names.size();
  S.files.resize(nfiles);
  S.file_rows.resize(nfiles);

  // open via cache + build the (file, col, rg) task list
  struct Task {
    size_t fi, c, rg;
  };
  std::vector<Task> tasks;
  for (size_t i = 0; i < nfiles; i++) {
    auto& fd = S.files[i];
    fd.f = FileCache::instance().open(paths[i]);
    S.file_rows[i] = fd.f->num_rows();
    fd.chunks.resize(names.size());
    fd.col_idx.resize(names.size());
    size_t nrg = fd.f->num_row_groups();
    for (size_t c = 0; c < names.size(); c++) {
      int ci = fd.f->column_index(names[c]);
      fd.col_idx[c] = ci;
      if (ci < 0) continue;
      fd.chunks[c].resize(nrg);
      for (size_t rg = 0; rg < nrg; rg++) tasks.push_back({i, c, rg});
    }
  }
  auto tp1 = now();
  {
    std::string err;
    std::mutex err_mu;
    ThreadPool::instance().parallel_for((int64_t)tasks.size(), [&](int64_t i) {
      try {
        const Task& t = tasks[i];
        auto& fd = S.files[t.fi];
        // hybrid host/GPU decompress split (profiles/r01_gpu_zstd.md
        // round-2 plan item 3): route gpu_zstd_frac of the chunks to the
        // GPU zstd kernel, the rest to the host pool — the prefetch
        // pipeline overlaps them across units, so steady-state unit cost
        // is max(host share, gpu share) instead of the loser's total
        bool this_gpu_zstd =
            gpu_zstd && ((double)((i * 2654435761u) % 1000) < gpu_zstd_frac * 1000.0);
        fd.chunks[t.c][t.rg] =
            fd.f->read_chunk(t.rg, fd.col_idx[t.c], gpu_snappy, true, this_gpu_zstd,
                             gpu_delta, gpu_huf, gpu_lz4, gpu_gzip);
      } catch (std::exception& e) {
        std::lock_guard<std::mutex> lk(err_mu);
        err = e.what();
      }
    });
    if (!err.empty()) throw std::runtime_error(err);
  }
  // the GPU decode route holds per (file, column): all of its chunks raw
  // in ONE encoding. Mixed encodings across row groups: host-decode the
  // raw chunks, and the column is a plain one.
  if (gpu_delta) {
    for (auto& fd : S.files) {
      for (size_t c = 0; c < names.size(); c++) {
        auto& chs = fd.chunks[c];
        if (chs.empty()) continue;  // the file lacks the column
        bool any = false, uniform = true;
        for (auto& ch : chs) {
          if (ch.enc_kind) any = true;
          if (ch.enc_kind != chs[0].enc_kind) uniform = false;
        }
        if (!any || uniform) continue;
        for (size_t rg = 0; rg < chs.size(); rg++)
          if (chs[rg].enc_kind)
            chs[rg] = fd.f->read_chunk(rg, fd.col_idx[c], false, false, false, false);
      }
    }
  }
  // likewise a column is dictionary-decoded only when all of its chunks
  // are: next to a plain chunk (a row group that fell back, or was
  // host-decoded above) the dictionary chunks turn plain on the host
  // (such a column is marked: it stays off the GPU string route)
  std::vector<char> mixed_dict(nfiles * names.size(), 0);
  for (size_t fi = 0; fi < nfiles; fi++) {
    auto& fd = S.files[fi];
    for (size_t c = 0; c < names.size(); c++) {
      if (fd.col_idx[c] < 0 || fd.f->columns()[fd.col_idx[c]].is_list) continue;
      bool any_dict = false, any_plain = false;
      for (auto& ch : fd.chunks[c]) {
        if (ch.is_dict) any_dict = true;
        else if (ch.num_values > ch.null_count) any_plain = true;
      }
      if (!(any_dict && any_plain)) continue;
      mixed_dict[fi * names.size() + c] = 1;
      for (auto& ch : fd.chunks[c])
        if (ch.is_dict) ParquetFile::undict_chunk(ch);
    }
  }
  auto tp2 = now();
  S.t_open_us = us(tp0, tp1);
  S.t_chunks_us = us(tp1, tp2);

  // layout
  S.str_cols.resize(nfiles * names.size());
  int64_t vpos = 0, vapos = 0, dpos = 0, spos = 0;
  int64_t huf_comp = 0;  // bytes of Huffman-only frames, LZ4 blocks and GZIP
                         // pages so far
  for (size_t fi = 0; fi < nfiles; fi++) {
    auto& fd = S.files[fi];
    for (size_t c = 0; c < names.size(); c++) {
      UnitColumn uc;
      uc.file_idx = (int)fi;
      uc.name = names[c];
      if (fd.col_idx[c] < 0) {
        S.cols.push_back(uc);
        continue;
      }
      uc.present = true;
      const ColumnDesc& cd = fd.f->columns()[fd.col_idx[c]];
      uc.physical = cd.physical;
      uc.is_list = cd.is_list;
      uc.is_string = !cd.is_list && cd.physical == PT_BYTE_ARRAY;
      auto& chs = fd.chunks[c];
      if (uc.is_list) {
        // rows (not element slots) are the unit currency for lists;
        // payload layout happens in the decoded pre-pass below (same
        // host-decode lane as strings)
        int64_t rows = 0;
        for (auto& ch : chs)
          rows += ch.list_offsets.empty() ? 0
                  : (int64_t)ch.list_offsets.size() - 1;
        uc.num_values = rows;
        bool any_null_row = false;
        for (auto& ch : chs)
          for (auto v : ch.list_validity)
            if (!v) any_null_row = true;
        uc.null_count = 0;
        for (auto& ch : chs) {
          size_t rows_c = ch.list_offsets.empty() ? 0 : ch.list_offsets.size() - 1;
          for (size_t i = 0; i < rows_c && i < ch.list_validity.size(); i++)
            if (!ch.list_validity[i]) uc.null_count++;
        }
        if (any_null_row) {
          uc.validity_off = vapos;
          vapos += rows;
        }
        uc.soff_off = spos;
        spos += rows + 1;
        S.cols.push_back(uc);
        continue;
      }
      int64_t nv = 0, nulls = 0;
      bool any_dict = false, any_valid = false;
      for (auto& ch : chs) {
        nv += ch.num_values;
        nulls += ch.null_count;
        if (ch.is_dict) any_dict = true;
        if (!ch.validity.empty()) any_valid = true;
      }
      uc.num_values = nv;
      uc.null_count = nulls;
      uc.is_dict = any_dict;
      if (any_valid) {
        uc.validity_off = vapos;
        vapos += nv;
      }
      if (!chs.empty() && chs[0].enc_kind) {
        // raw DELTA_BINARY_PACKED / BYTE_STREAM_SPLIT pages (every chunk,
        // same kind: see the fix-up above): page and miniblock rows
        uc.enc = chs[0].enc_kind;
        uc.val_off = vpos;
        int es = physical_elem_size(uc.physical);
        std::vector<int64_t> pages, mbs;
        int64_t poff = uc.val_off, dense_off = 0;
        for (auto& ch : chs) {
          for (auto& ep : ch.enc_pages) {
            int64_t abs_off = poff + ep.payload_off;
            int64_t page_row = (int64_t)pages.size() / 6;
            if (uc.enc == ParquetFile::ENCK_BYTE_STREAM_SPLIT) {
              if (ep.n > 0 && ep.n > ep.payload_len / es)
                throw std::runtime_error(
                    "byte-stream-split: page shorter than its values");
              pages.insert(pages.end(), {dense_off, ep.n, abs_off, 0, 0, 0});
            } else {
              DeltaHeader h;
              int64_t first_mb = (int64_t)mbs.size() / 6;
              int64_t carried = 0;
              if (ep.n > 0) {
                delta_walk(ch.values.data() + ep.payload_off,
                           (size_t)ep.payload_len, es * 8, (uint64_t)ep.n, h,
                           [&](const DeltaMiniblock& m) {
                  mbs.insert(mbs.end(),
                             {dense_off + m.first, m.n, abs_off * 8 + m.bit_off,
                              (int64_t)m.bit_width, (int64_t)m.min_delta,
                              page_row});
                  carried += m.n;
                });
                if ((int64_t)h.count != ep.n || carried + 1 != ep.n)
                  throw std::runtime_error(
                      "delta: stream holds fewer values than the page");
              }
              pages.insert(pages.end(), {dense_off, ep.n,
                                         (int64_t)h.first_value, first_mb, 0, 0});
            }
            dense_off += ep.n;
          }
          poff += ru_align8((int64_t)ch.values.size());
        }
        uc.val_len = poff - uc.val_off + 8;
        vpos += uc.val_len;
        uc.dense_n = dense_off;
        uc.enc_off = (int64_t)S.enc.size() / 6;
        uc.enc_pages = (int64_t)pages.size() / 6;
        S.enc.insert(S.enc.end(), pages.begin(), pages.end());
        S.enc.insert(S.enc.end(), mbs.begin(), mbs.end());
        uc.enc_cnt = (int64_t)S.enc.size() / 6 - uc.enc_off;
      } else if (uc.is_string && gpu_strings && cd.max_def <= 1 &&
                 cd.physical == PT_BYTE_ARRAY &&
                 cd.name.find('.') == std::string::npos &&
                 !mixed_dict[fi * names.size() + c]) {
        // GPU string route (after the fix-up above the chunks with stored
        // values are all dictionary chunks or all plain ones)
        uc.soff_off = spos;
        uc.sbytes_off = -1;
        int64_t dense = 0;
        for (auto& ch : chs) dense += ch.num_values - ch.null_count;
        uc.dense_n = dense;
        if (!uc.is_dict) {
          // the walk of the prefixes runs in the pre-pass below
          uc.str_kind = UD_STR_PLAIN;
          uc.val_off = vpos;
          int64_t plen = 0;
          for (auto& ch : chs) plen += (int64_t)ch.values.size();
          uc.val_len = plen;
          vpos += ru_align8(plen);
          spos += dense + 1;
        } else {
          uc.str_kind = UD_STR_DICT;
          uc.val_off = vpos;
          auto sd = std::make_unique<UnitStage::StrDecoded>();
          sd->offs.push_back(0);
          uc.run_off = (int64_t)S.runs.size() / 6;
          int64_t poff = uc.val_off, dense_off = 0, bias = 0, dbytes = 0;
          for (auto& ch : chs) {
            if (ch.is_dict)
              str_walk_dict(ch.dict.data(), ch.dict.size(), ch.dict_num_values,
                            dbytes, sd->offs, sd->bytes);
            for (auto& ip : ch.idx_pages) {
              std::vector<RleRun> rr;
              parse_rle_runs(ch.values.data() + ip.payload_off,
                             (size_t)ip.payload_len, ip.bit_width, ip.n,
                             (poff + ip.payload_off) * 8, rr);
              for (auto& r : rr) {
                if (!r.is_literal && r.n > 0 &&
                    (int64_t)r.value >= ch.dict_num_values)
                  throw std::runtime_error("dictionary index out of range");
                S.runs.push_back(r.out_off + dense_off);
                S.runs.push_back(r.n);
                S.runs.push_back(r.is_literal);
                S.runs.push_back(r.is_literal ? r.bit_off : (int64_t)r.value + bias);
                S.runs.push_back(ip.bit_width);
                S.runs.push_back(bias);
              }
              dense_off += ip.n;
            }
            poff += ru_align8((int64_t)ch.values.size());
            if (ch.is_dict) bias += ch.dict_num_values;
          }
          if (dense_off != dense)
            throw std::runtime_error(
                "dictionary index pages hold another count than the chunks");
          uc.val_len = poff - uc.val_off + 8;
          vpos += uc.val_len;
          uc.run_cnt = (int64_t)S.runs.size() / 6 - uc.run_off;
          uc.dict_off = dpos;
          uc.dict_len = (int64_t)sd->bytes.size();
          dpos += ru_align8(uc.dict_len);
          uc.sbytes_len = (int64_t)sd->offs.size() - 1;  // entries
          spos += (int64_t)sd->offs.size();
          S.str_cols[fi * names.size() + c] = std::move(sd);
        }
      } else if (uc.is_string) {
        uc.soff_off = spos;
        spos += nv + 1;
      } else if (uc.is_dict) {
        uc.val_off = vpos;
        int64_t plen = 0, dlen = 0, dense = 0;
        for (auto& ch : chs) {
          plen += ru_align8((int64_t)ch.values.size());
          dlen += ru_align8((int64_t)ch.dict.size());
          dense += ch.num_values - ch.null_count;
        }
        uc.val_len = plen + 8;
        vpos += uc.val_len;
        uc.dict_off = dpos;
        uc.dict_len = dlen;
        dpos += dlen;
        uc.dense_n = dense;
        // runs (bit offsets are relative to the values buffer)
        uc.run_off = (int64_t)S.runs.size() / 6;
        int64_t poff = uc.val_off;
        int64_t dense_off = 0;
        int64_t bias = 0;
        int es = physical_elem_size(uc.physical);
        for (auto& ch : chs) {
          for (auto& ip : ch.idx_pages) {
            std::vector<RleRun> rr;
            parse_rle_runs(ch.values.data() + ip.payload_off,
                           (size_t)ip.payload_len, ip.bit_width, ip.n,
                           (poff + ip.payload_off) * 8, rr);
            for (auto& r : rr) {
              S.runs.push_back(r.out_off + dense_off);
              S.runs.push_back(r.n);
              S.runs.push_back(r.is_literal);
              S.runs.push_back(r.is_literal ? r.bit_off : (int64_t)r.value + bias);
              S.runs.push_back(ip.bit_width);
              S.runs.push_back(bias);
            }
            dense_off += ip.n;
          }
          poff += ru_align8((int64_t)ch.values.size());
          bias += (int64_t)(ru_align8((int64_t)ch.dict.size()) / es);
        }
        uc.run_cnt = (int64_t)S.runs.size() / 6 - uc.run_off;
      } else {
        uc.val_off = vpos;
        int64_t plen = 0;
        for (auto& ch : chs) {
          // (huf_pages is empty unless the chunk is gpu_compressed or
          // host_deferred; their frames follow everything else in comp)
          for (auto& hp : ch.huf_pages) {
            S.huf_jobs.insert(S.huf_jobs.end(),
                              {huf_comp, hp.comp_len, vpos + plen + hp.out_off,
                               hp.out_len});
            S.huf_src.push_back(
                {(int)fi, hp.file_off, hp.comp_len, huf_comp, hp.out_len, hp.codec});
            huf_comp += hp.comp_len;
          }
          for (auto& lp : ch.lz4_pages) {
            S.lz4_jobs.insert(S.lz4_jobs.end(),
                              {huf_comp, lp.comp_len, vpos + plen + lp.out_off,
                               lp.out_len});
            S.lz4_src.push_back(
                {(int)fi, lp.file_off, lp.comp_len, huf_comp, lp.out_len, lp.codec});
            huf_comp += lp.comp_len;
          }
          for (auto& gp : ch.gzip_pages) {
            S.gzip_jobs.insert(S.gzip_jobs.end(),
                               {huf_comp, gp.comp_len, vpos + plen + gp.out_off,
                                gp.out_len});
            S.gzip_src.push_back(
                {(int)fi, gp.file_off, gp.comp_len, huf_comp, gp.out_len, gp.codec});
            huf_comp += gp.comp_len;
          }
          if (ch.gpu_compressed) {
            for (auto& cp : ch.comp_pages) {
              auto& jobs = (cp.codec == CODEC_ZSTD) ? S.zstd_jobs : S.snappy_jobs;
              jobs.push_back(S.comp_size + cp.comp_off);
              jobs.push_back(cp.comp_len);
              jobs.push_back(vpos + plen + cp.out_off);
              jobs.push_back(cp.out_len);
            }
            S.comp_size += (int64_t)ch.comp.size();
            plen += ch.values_len;
          } else if (ch.host_deferred) {
            for (auto& dp : ch.defer_pages) {
              S.host_jobs.push_back(
                  {(int)fi, dp.file_off, dp.comp_len, vpos + plen + dp.out_off,
                   dp.out_len, dp.codec});
            }
            plen += ch.values_len;
          } else {
            plen += (int64_t)ch.values.size();
          }
        }
        uc.val_len = plen;
        vpos += ru_align8(plen);
      }
      S.cols.push_back(uc);
    }
  }

  // string pre-pass (decode to learn byte totals) — parallel per column
  {
    std::vector<size_t> str_idx;
    for (size_t u = 0; u < S.cols.size(); u++)
      if (S.cols[u].present && (S.cols[u].is_string || S.cols[u].is_list) &&
          S.cols[u].str_kind != UD_STR_DICT)
        str_idx.push_back(u);
    std::string err;
    std::mutex err_mu;
    ThreadPool::instance().parallel_for((int64_t)str_idx.size(), [&](int64_t k) {
      try {
        size_t u = str_idx[k];
        UnitColumn& uc = S.cols[u];
        auto& fd = S.files[uc.file_idx];
        auto sd = std::make_unique<UnitStage::StrDecoded>();
        sd->offs.push_back(0);
        if (uc.str_kind == UD_STR_PLAIN) {
          // prefixes only: the payload is not touched on the host
          int64_t total = 0;
          sd->offs.reserve((size_t)uc.dense_n + 1);
          for (auto& ch : fd.chunks[u % S.ncols])
            str_walk_plain(ch.values.data(), ch.values.size(),
                           ch.num_values - ch.null_count, total, sd->offs);
        } else if (uc.is_list) {
          int es = physical_elem_size(uc.physical);
          for (auto& ch : fd.chunks[u % S.ncols]) {
            DecodedColumn dc = decode_chunk_cpu(ch);
            int64_t elem_base = (int64_t)sd->bytes.size() / es;
            sd->bytes.insert(sd->bytes.end(), dc.data.begin(), dc.data.end());
            for (size_t i = 1; i < dc.list_offsets.size(); i++)
              sd->offs.push_back(elem_base + dc.list_offsets[i]);
            size_t rows = dc.list_offsets.empty()
                              ? 0 : dc.list_offsets.size() - 1;
            if (!dc.list_validity.empty())
              sd->row_valid.insert(sd->row_valid.end(),
                                   dc.list_validity.begin(),
                                   dc.list_validity.begin() + rows);
            else
              sd->row_valid.insert(sd->row_valid.end(), rows, 1);
          }
        } else {
          for (auto& ch : fd.chunks[u % S.ncols]) {
            DecodedColumn dc = decode_chunk_cpu(ch);
            int64_t base = (int64_t)sd->bytes.size();
            sd->bytes.insert(sd->bytes.end(), dc.bytes.begin(), dc.bytes.end());
            for (size_t i = 1; i < dc.offsets.size(); i++)
              sd->offs.push_back(base + dc.offsets[i]);
          }
        }
        S.str_cols[u] = std::move(sd);
      } catch (std::exception& e) {
        std::lock_guard<std::mutex> lk(err_mu);
        err = e.what();
      }
    });
    if (!err.empty()) throw std::runtime_error(err);
    for (size_t u : str_idx) {
      UnitColumn& uc = S.cols[u];
      if (uc.str_kind == UD_STR_PLAIN) {
        uc.sbytes_len = S.str_cols[u]->offs.back();
        continue;
      }
      uc.sbytes_off = vpos;
      uc.sbytes_len = (int64_t)S.str_cols[u]->bytes.size();
      vpos += ru_align8(uc.sbytes_len);
    }
  }

  // the Huffman-only frames, the LZ4 blocks and the GZIP pages go behind
  // the chunk-owned page bodies in comp
  for (size_t i = 0; i < S.huf_src.size(); i++) {
    S.huf_jobs[4 * i] += S.comp_size;
    S.huf_src[i].dst_off += S.comp_size;
  }
  for (size_t i = 0; i < S.lz4_src.size(); i++) {
    S.lz4_jobs[4 * i] += S.comp_size;
    S.lz4_src[i].dst_off += S.comp_size;
  }
  for (size_t i = 0; i < S.gzip_src.size(); i++) {
    S.gzip_jobs[4 * i] += S.comp_size;
    S.gzip_src[i].dst_off += S.comp_size;
  }
  S.comp_size += huf_comp;

  S.values_size = vpos;
  S.validity_size = vapos;
  S.dicts_size = dpos;
  S.soffs_size = spos;
  S.t_layout_us = us(tp2, now());
  return st;
}

// Fill caller-allocated buffers (sized from stage1) — pure parallel memcpy.
inline void read_unit_fill(UnitStage& S, uint8_t* values, uint8_t* validity,
                           uint8_t* dicts, int64_t* soffs, uint8_t* comp) {
  // compressed snappy page bodies, in the same chunk order the layout
  // assigned (serial: tiny relative to values)
  if (comp) {
    int64_t cpos = 0;
    for (size_t u = 0; u < S.cols.size(); u++) {
      UnitColumn& uc = S.cols[u];
      if (!uc.present || uc.is_string || uc.is_dict) continue;
      auto& chs = S.files[uc.file_idx].chunks[u % S.ncols];
      for (auto& ch : chs) {
        if (ch.gpu_compressed && !ch.comp.empty()) {
          std::memcpy(comp + cpos, ch.comp.data(), ch.comp.size());
          cpos += (int64_t)ch.comp.size();
        }
      }
    }
  }
  if (S.validity_size) std::memset(validity, 1, (size_t)S.validity_size);
  ThreadPool::instance().parallel_for((int64_t)S.cols.size(), [&](int64_t u) {
    UnitColumn& uc = S.cols[u];
    if (!uc.present) return;
    auto& fd = S.files[uc.file_idx];
    auto& chs = fd.chunks[u % S.ncols];
    if (uc.validity_off >= 0 && !uc.is_list) {
      int64_t off = uc.validity_off;
      for (auto& ch : chs) {
        if (!ch.validity.empty())
          std::memcpy(validity + off, ch.validity.data(), ch.validity.size());
        off += ch.num_values;
      }
    }
    if (uc.str_kind != UD_STR_HOST) {
      auto& sd = *S.str_cols[u];
      std::memcpy(soffs + uc.soff_off, sd.offs.data(), sd.offs.size() * 8);
      int64_t poff = uc.val_off;
      for (auto& ch : chs) {
        if (!ch.values.empty())
          std::memcpy(values + poff, ch.values.data(), ch.values.size());
        poff += uc.str_kind == UD_STR_PLAIN ? (int64_t)ch.values.size()
                                            : ru_align8((int64_t)ch.values.size());
      }
      if (!sd.bytes.empty())
        std::memcpy(dicts + uc.dict_off, sd.bytes.data(), sd.bytes.size());
      return;
    }
    if (uc.is_string || uc.is_list) {
      auto& sd = *S.str_cols[u];
      std::memcpy(soffs + uc.soff_off, sd.offs.data(), sd.offs.size() * 8);
      if (!sd.bytes.empty())
        std::memcpy(values + uc.sbytes_off, sd.bytes.data(), sd.bytes.size());
      if (uc.is_list && uc.validity_off >= 0 && !sd.row_valid.empty())
        std::memcpy(validity + uc.validity_off, sd.row_valid.data(),
                    sd.row_valid.size());
      return;
    }
    if (uc.enc) {
      int64_t poff = uc.val_off;
      for (auto& ch : chs) {
        if (!ch.values.empty())
          std::memcpy(values + poff, ch.values.data(), ch.values.size());
        poff += ru_align8((int64_t)ch.values.size());
      }
      return;
    }
    if (uc.is_dict) {
      int64_t poff = uc.val_off;
      int64_t doff = uc.dict_off;
      for (auto& ch : chs) {
        std::memcpy(values + poff, ch.values.data(), ch.values.size());
        std::memcpy(dicts + doff, ch.dict.data(), ch.dict.size());
        poff += ru_align8((int64_t)ch.values.size());
        doff += ru_align8((int64_t)ch.dict.size());
      }
      return;
    }
    int64_t off = uc.val_off;
    for (auto& ch : chs) {
      if (ch.gpu_compressed || ch.host_deferred) {
        off += ch.values_len;  // GPU snappy kernel / host job fills it
        continue;
      }
      std::memcpy(values + off, ch.values.data(), ch.values.size());
      off += (int64_t)ch.values.size();
    }
  });
  // deferred pages: decompress straight from the file mmap into the
  // destination buffer (one pass, zero staging)
  // and, in the same sweep of the pool, the frames of the Huffman-only
  // pages, the LZ4 blocks and the GZIP pages from the mmap into comp for
  // the GPU (tens of MB per unit: not for the serial copy above)
  const int64_t nhost = (int64_t)S.host_jobs.size();
  const int64_t nhuf = comp ? (int64_t)S.huf_src.size() : 0;
  const int64_t nlz4 = comp ? (int64_t)S.lz4_src.size() : 0;
  const int64_t ngzip = comp ? (int64_t)S.gzip_src.size() : 0;
  ThreadPool::instance().parallel_for(nhost + nhuf + nlz4 + ngzip, [&](int64_t i) {
    if (i >= nhost) {
      const UnitStage::HostJob& hs =
          i - nhost < nhuf          ? S.huf_src[i - nhost]
          : i - nhost - nhuf < nlz4 ? S.lz4_src[i - nhost - nhuf]
                                    : S.gzip_src[i - nhost - nhuf - nlz4];
      std::memcpy(comp + hs.dst_off,
                  S.files[hs.file_idx].f->data_at(hs.file_off),
                  (size_t)hs.comp_len);
      return;
    }
    const UnitStage::HostJob& hj = S.host_jobs[i];
    const uint8_t* src = S.files[hj.file_idx].f->data_at(hj.file_off);
    decompress_into(hj.codec, values + hj.dst_off, (size_t)hj.dst_len, src,
                    (size_t)hj.comp_len);
  });
}

}  // namespace lakesoul
