// lakesoul_amd._cpp — host-side native core: parquet read/write, spark
// murmur3, CPU decode fallbacks. GPU kernels live in lakesoul_amd._hip.
#include <torch/extension.h>

#include <atomic>
#include <cstring>
#include <memory>
#include <map>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <chrono>

#include "merge_plan.h"
#include "murmur3.h"
#include "parquet_file.h"
#include "read_unit.h"
#include "str_pred.h"
#include "str_seg.h"
#include "str_walk.h"
#include "unit_desc.h"
#include "huf_par.h"
#include "zstd_dec.h"

namespace py = pybind11;
using namespace lakesoul;

// ---------------------------------------------------------------------- //
// dtype mapping: canonical dtype string <-> parquet physical/logical
// ---------------------------------------------------------------------- //

struct DtypeInfo {
  int32_t physical;
  int32_t converted;
  LogicalTag logical;
  int32_t bit_width;
  int32_t dec_precision = 0;
  int32_t dec_scale = 0;
};

static DtypeInfo dtype_info(const std::string& dt) {
  if (dt == "bool") return {PT_BOOLEAN, CV_NONE, LogicalTag::NONE, 0};
  if (dt == "int8") return {PT_INT32, CV_INT_8, LogicalTag::INT, 8};
  if (dt == "int16") return {PT_INT32, CV_INT_16, LogicalTag::INT, 16};
  if (dt == "int32") return {PT_INT32, CV_NONE, LogicalTag::NONE, 0};
  if (dt == "int64") return {PT_INT64, CV_NONE, LogicalTag::NONE, 0};
  if (dt == "float32") return {PT_FLOAT, CV_NONE, LogicalTag::NONE, 0};
  if (dt == "float64") return {PT_DOUBLE, CV_NONE, LogicalTag::NONE, 0};
  if (dt == "string") return {PT_BYTE_ARRAY, CV_UTF8, LogicalTag::STRING, 0};
  if (dt == "binary") return {PT_BYTE_ARRAY, CV_NONE, LogicalTag::NONE, 0};
  if (dt == "date32") return {PT_INT32, CV_DATE, LogicalTag::DATE, 0};
  if (dt == "timestamp[ms]")
    return {PT_INT64, CV_TIMESTAMP_MILLIS, LogicalTag::TIMESTAMP_MILLIS, 0};
  if (dt == "timestamp[us]")
    return {PT_INT64, CV_TIMESTAMP_MICROS, LogicalTag::TIMESTAMP_MICROS, 0};
  if (dt == "timestamp[ns]")
    return {PT_INT64, CV_NONE, LogicalTag::TIMESTAMP_NANOS, 0};
  if (dt.rfind("decimal(", 0) == 0 && dt.back() == ')') {
    // decimal(p,s), p<=18: stored as INT64 unscaled (parquet spec allows
    // INT32/INT64 physical for small precisions; arrow reads it with
    // store_decimal_as_integer parity)
    int p = 0, sc = 0;
    if (sscanf(dt.c_str(), "decimal(%d,%d)", &p, &sc) != 2 || p <= 0 || p > 18)
      throw std::runtime_error("unsupported decimal dtype: " + dt);
    DtypeInfo di{PT_INT64, CV_DECIMAL, LogicalTag::DECIMAL, 0};
    di.dec_precision = p;
    di.dec_scale = sc;
    return di;
  }
  throw std::runtime_error("unsupported dtype: " + dt);
}

static std::string dtype_name_scalar(const ColumnDesc& c) {
  switch (c.physical) {
    case PT_BOOLEAN:
      return "bool";
    case PT_INT32:
      if (c.converted == CV_INT_8 || (c.logical == LogicalTag::INT && c.int_bit_width == 8))
        return "int8";
      if (c.converted == CV_INT_16 || (c.logical == LogicalTag::INT && c.int_bit_width == 16))
        return "int16";
      if (c.converted == CV_DATE || c.logical == LogicalTag::DATE) return "date32";
      return "int32";
    case PT_INT64:
      if (c.converted == CV_DECIMAL || c.logical == LogicalTag::DECIMAL)
        return "decimal(" + std::to_string(c.dec_precision) + "," +
               std::to_string(c.dec_scale) + ")";
      if (c.converted == CV_TIMESTAMP_MILLIS || c.logical == LogicalTag::TIMESTAMP_MILLIS)
        return "timestamp[ms]";
      if (c.converted == CV_TIMESTAMP_MICROS || c.logical == LogicalTag::TIMESTAMP_MICROS)
        return "timestamp[us]";
      if (c.logical == LogicalTag::TIMESTAMP_NANOS) return "timestamp[ns]";
      return "int64";
    case PT_FLOAT:
      return "float32";
    case PT_DOUBLE:
      return "float64";
    case PT_BYTE_ARRAY:
      if (c.converted == CV_UTF8 || c.logical == LogicalTag::STRING) return "string";
      return "binary";
    case PT_FLBA:
      return "binary";   // fixed-len values surface as binary cells
    case PT_INT96:
      return "timestamp[ns]";
    default:
      return "unsupported";
  }
}

// ---------------------------------------------------------------------- //
// writer binding
// ---------------------------------------------------------------------- //

static std::string dtype_name(const ColumnDesc& c) {
  if (c.is_list) return "list<" + dtype_name_scalar(c) + ">";
  return dtype_name_scalar(c);
}

static int64_t write_parquet(
    const std::string& path, const std::vector<std::string>& names,
    const std::vector<std::string>& dtypes, const std::vector<torch::Tensor>& columns,
    const std::vector<c10::optional<torch::Tensor>>& offsets,
    const std::vector<c10::optional<torch::Tensor>>& validity,
    const std::vector<bool>& nullable, int64_t row_group_size, int64_t codec,
    int64_t level,
    const std::vector<c10::optional<torch::Tensor>>& elem_offsets = {},
    const std::vector<std::string>& parents = {}) {
  size_t ncol = names.size();
  TORCH_CHECK(dtypes.size() == ncol && columns.size() == ncol);
  std::vector<ColumnDesc> descs(ncol);
  std::vector<ColumnData> data(ncol);
  int64_t num_rows = -1;
  std::vector<torch::Tensor> keep;  // hold contiguous refs

  for (size_t i = 0; i < ncol; i++) {
    bool is_list = dtypes[i].rfind("list<", 0) == 0;
    std::string scalar_dtype = is_list
        ? dtypes[i].substr(5, dtypes[i].size() - 6)
        : dtypes[i];
    DtypeInfo di = dtype_info(scalar_dtype);
    descs[i].name = names[i];
    descs[i].physical = di.physical;
    descs[i].converted = di.converted;
    descs[i].logical = di.logical;
    descs[i].int_bit_width = di.bit_width;
    descs[i].dec_precision = di.dec_precision;
    descs[i].dec_scale = di.dec_scale;
    descs[i].nullable = nullable[i];
    descs[i].is_list = is_list;
    if (is_list) {
      descs[i].max_def = 2;  // optional list group + repeated, required elem
    }
    if (i < parents.size() && !parents[i].empty()) {
      // "struct:NAME" / "map:NAME" — the enclosing group
      const std::string& p = parents[i];
      auto colon = p.find(':');
      TORCH_CHECK(colon != std::string::npos, "bad parent spec ", p);
      descs[i].parent = p.substr(colon + 1);
      descs[i].parent_kind = p.rfind("map", 0) == 0 ? 2 : 1;
    }

    torch::Tensor col = columns[i].contiguous().cpu();
    keep.push_back(col);
    if (is_list) {
      TORCH_CHECK(offsets[i].has_value(), "list column needs offsets");
      torch::Tensor off = offsets[i]->contiguous().cpu().to(torch::kInt64);
      keep.push_back(off);
      data[i].list_offsets = off.data_ptr<int64_t>();
      if (di.physical == PT_BYTE_ARRAY) {
        // list<string>: col = payload bytes, elem_offsets = element
        // byte offsets (int32)
        TORCH_CHECK(i < elem_offsets.size() && elem_offsets[i].has_value(),
                    "list<string> column needs elem_offsets");
        torch::Tensor eo = elem_offsets[i]->contiguous().cpu().to(torch::kInt32);
        keep.push_back(eo);
        data[i].offsets = eo.data_ptr<int32_t>();
        data[i].bytes = (const uint8_t*)col.data_ptr();
      } else {
        data[i].data = (const uint8_t*)col.data_ptr();
        int es = physical_elem_size(di.physical);
        TORCH_CHECK(col.element_size() == es, "list element size mismatch");
      }
      int64_t n = off.numel() - 1;
      TORCH_CHECK(num_rows < 0 || n == num_rows, "row count mismatch");
      num_rows = n;
    } else if (di.physical == PT_BYTE_ARRAY) {
      TORCH_CHECK(offsets[i].has_value(), "byte_array column needs offsets");
      torch::Tensor off = offsets[i]->contiguous().cpu().to(torch::kInt32);
      keep.push_back(off);
      data[i].offsets = off.data_ptr<int32_t>();
      data[i].bytes = (const uint8_t*)col.data_ptr();
      int64_t n = off.numel() - 1;
      TORCH_CHECK(num_rows < 0 || n == num_rows, "row count mismatch");
      num_rows = n;
    } else {
      // dtype check: int8/int16 must be passed widened to int32
      data[i].data = (const uint8_t*)col.data_ptr();
      int64_t n = col.numel();
      TORCH_CHECK(num_rows < 0 || n == num_rows, "row count mismatch");
      num_rows = n;
      int es = physical_elem_size(di.physical);
      TORCH_CHECK(col.element_size() == es, "column ", names[i],
                  " element size ", col.element_size(), " != physical ", es);
    }
    if (validity[i].has_value()) {
      torch::Tensor v = validity[i]->contiguous().cpu().to(torch::kUInt8);
      keep.push_back(v);
      data[i].validity = v.data_ptr<uint8_t>();
    }
  }
  if (num_rows < 0) num_rows = 0;

  int64_t size;
  {
    py::gil_scoped_release rel;
    ParquetWriter w(path, descs, (int)codec, (int)level, row_group_size);
    w.write_row_group(data, num_rows);
    size = w.close();
  }
  return size;
}

// ---------------------------------------------------------------------- //
// incremental writer handles (streaming multipart upload support):
// writer_open -> write batches one by one (each call appends row groups
// and flushes) -> writer_bytes gives the stable part boundary ->
// writer_finish emits the footer. The marshaling mirrors write_parquet.
// ---------------------------------------------------------------------- //

namespace {
struct OpenWriter {
  std::unique_ptr<ParquetWriter> w;
  std::vector<ColumnDesc> descs;
  std::vector<std::string> dtypes;
  std::string path;
};
std::mutex g_wmu;
std::map<int64_t, std::shared_ptr<OpenWriter>> g_writers;
int64_t g_wnext = 1;

std::shared_ptr<OpenWriter> get_writer(int64_t h) {
  std::lock_guard<std::mutex> lk(g_wmu);
  auto it = g_writers.find(h);
  if (it == g_writers.end()) throw std::runtime_error("bad writer handle");
  return it->second;
}
}  // namespace

static int64_t writer_open(const std::string& path,
                           const std::vector<std::string>& names,
                           const std::vector<std::string>& dtypes,
                           const std::vector<bool>& nullable,
                           int64_t row_group_size, int64_t codec,
                           int64_t level,
                           const std::vector<std::string>& parents = {}) {
  auto ow = std::make_shared<OpenWriter>();
  ow->path = path;
  ow->dtypes = dtypes;
  ow->descs.resize(names.size());
  for (size_t i = 0; i < names.size(); i++) {
    bool is_list = dtypes[i].rfind("list<", 0) == 0;
    std::string sd = is_list ? dtypes[i].substr(5, dtypes[i].size() - 6)
                             : dtypes[i];
    DtypeInfo di = dtype_info(sd);
    ColumnDesc& d = ow->descs[i];
    d.name = names[i];
    d.physical = di.physical;
    d.converted = di.converted;
    d.logical = di.logical;
    d.int_bit_width = di.bit_width;
    d.dec_precision = di.dec_precision;
    d.dec_scale = di.dec_scale;
    d.nullable = nullable[i];
    d.is_list = is_list;
    if (is_list) d.max_def = 2;
    if (i < parents.size() && !parents[i].empty()) {
      const std::string& p = parents[i];
      auto colon = p.find(':');
      TORCH_CHECK(colon != std::string::npos, "bad parent spec ", p);
      d.parent = p.substr(colon + 1);
      d.parent_kind = p.rfind("map", 0) == 0 ? 2 : 1;
    }
  }
  ow->w = std::make_unique<ParquetWriter>(path, ow->descs, (int)codec,
                                          (int)level, row_group_size);
  std::lock_guard<std::mutex> lk(g_wmu);
  int64_t h = g_wnext++;
  g_writers[h] = ow;
  return h;
}

static void writer_write(int64_t h, const std::vector<torch::Tensor>& columns,
                         const std::vector<c10::optional<torch::Tensor>>& offsets,
                         const std::vector<c10::optional<torch::Tensor>>& validity,
                         const std::vector<c10::optional<torch::Tensor>>& elem_offsets = {}) {
  auto ow = get_writer(h);
  size_t ncol = ow->descs.size();
  TORCH_CHECK(columns.size() == ncol);
  std::vector<ColumnData> data(ncol);
  std::vector<torch::Tensor> keep;
  int64_t num_rows = -1;
  for (size_t i = 0; i < ncol; i++) {
    const ColumnDesc& d = ow->descs[i];
    torch::Tensor col = columns[i].contiguous().cpu();
    keep.push_back(col);
    if (d.is_list) {
      TORCH_CHECK(offsets[i].has_value(), "list column needs offsets");
      torch::Tensor off = offsets[i]->contiguous().cpu().to(torch::kInt64);
      keep.push_back(off);
      data[i].list_offsets = off.data_ptr<int64_t>();
      if (d.physical == PT_BYTE_ARRAY) {
        TORCH_CHECK(i < elem_offsets.size() && elem_offsets[i].has_value(),
                    "list<string> column needs elem_offsets");
        torch::Tensor eo = elem_offsets[i]->contiguous().cpu().to(torch::kInt32);
        keep.push_back(eo);
        data[i].offsets = eo.data_ptr<int32_t>();
        data[i].bytes = (const uint8_t*)col.data_ptr();
      } else {
        data[i].data = (const uint8_t*)col.data_ptr();
      }
      int64_t n = off.numel() - 1;
      TORCH_CHECK(num_rows < 0 || n == num_rows);
      num_rows = n;
    } else if (d.physical == PT_BYTE_ARRAY) {
      TORCH_CHECK(offsets[i].has_value(), "byte_array column needs offsets");
      torch::Tensor off = offsets[i]->contiguous().cpu().to(torch::kInt32);
      keep.push_back(off);
      data[i].offsets = off.data_ptr<int32_t>();
      data[i].bytes = (const uint8_t*)col.data_ptr();
      int64_t n = off.numel() - 1;
      TORCH_CHECK(num_rows < 0 || n == num_rows);
      num_rows = n;
    } else {
      data[i].data = (const uint8_t*)col.data_ptr();
      int64_t n = col.numel();
      TORCH_CHECK(num_rows < 0 || n == num_rows);
      num_rows = n;
    }
    if (validity[i].has_value()) {
      torch::Tensor v = validity[i]->contiguous().cpu().to(torch::kUInt8);
      keep.push_back(v);
      data[i].validity = v.data_ptr<uint8_t>();
    }
  }
  if (num_rows < 0) num_rows = 0;
  py::gil_scoped_release rel;
  ow->w->write_row_group(data, num_rows);
  ow->w->flush_os();
}

static int64_t writer_bytes(int64_t h) { return get_writer(h)->w->bytes_written(); }

static int64_t writer_finish(int64_t h) {
  auto ow = get_writer(h);
  int64_t size;
  {
    py::gil_scoped_release rel;
    size = ow->w->close();
  }
  std::lock_guard<std::mutex> lk(g_wmu);
  g_writers.erase(h);
  return size;
}

static void writer_abort(int64_t h) {
  std::shared_ptr<OpenWriter> ow;
  {
    std::lock_guard<std::mutex> lk(g_wmu);
    auto it = g_writers.find(h);
    if (it == g_writers.end()) return;
    ow = it->second;
    g_writers.erase(it);
  }
  ow->w.reset();
  std::remove(ow->path.c_str());
}

// ---------------------------------------------------------------------- //
// reader bindings
// ---------------------------------------------------------------------- //

static std::unordered_map<int64_t, std::shared_ptr<ParquetFile>> g_files;
static std::mutex g_files_mu;
static std::atomic<int64_t> g_next_handle{1};

static int64_t open_parquet(const std::string& path) {
  auto f = std::make_shared<ParquetFile>(path);
  std::lock_guard<std::mutex> lk(g_files_mu);
  int64_t h = g_next_handle++;
  g_files[h] = f;
  return h;
}

static std::shared_ptr<ParquetFile> get_file(int64_t h) {
  std::lock_guard<std::mutex> lk(g_files_mu);
  auto it = g_files.find(h);
  TORCH_CHECK(it != g_files.end(), "bad parquet handle");
  return it->second;
}

static void close_parquet(int64_t h) {
  std::lock_guard<std::mutex> lk(g_files_mu);
  g_files.erase(h);
}

static py::dict parquet_meta(int64_t h) {
  auto f = get_file(h);
  py::dict d;
  d["num_rows"] = f->num_rows();
  d["num_row_groups"] = (int64_t)f->num_row_groups();
  py::list cols;
  for (auto& c : f->columns()) {
    py::dict cd;
    cd["name"] = c.name;
    cd["dtype"] = dtype_name(c);
    cd["nullable"] = c.nullable;
    cols.append(cd);
  }
  d["columns"] = cols;
  py::list rgs;
  for (auto& g : f->meta().row_groups) {
    py::dict gd;
    gd["num_rows"] = g.num_rows;
    py::list cstats;
    for (auto& cm : g.columns) {
      py::dict sd;
      sd["num_values"] = cm.num_values;
      sd["null_count"] = cm.stats.null_count;
      if (cm.stats.has_min_max) {
        sd["min"] = py::bytes(cm.stats.min_value);
        sd["max"] = py::bytes(cm.stats.max_value);
      }
      cstats.append(sd);
    }
    gd["columns"] = cstats;
    rgs.append(gd);
  }
  d["row_groups"] = rgs;
  return d;
}

static torch::Tensor vec_to_tensor_u8(std::vector<uint8_t>&& v) {
  auto t = torch::empty({(int64_t)v.size()}, torch::kUInt8);
  std::memcpy(t.data_ptr(), v.data(), v.size());
  return t;
}

static torch::Tensor vec_to_tensor_i32(std::vector<int32_t>&& v) {
  auto t = torch::empty({(int64_t)v.size()}, torch::kInt32);
  std::memcpy(t.data_ptr(), v.data(), v.size() * 4);
  return t;
}

// raw chunk for GPU decode
static py::dict chunk_to_dict_raw(ParquetFile::ChunkData&& ch) {
  py::dict d;
  d["physical"] = ch.physical;
  d["num_values"] = ch.num_values;
  d["null_count"] = ch.null_count;
  d["is_dict"] = ch.is_dict;
  d["dict_num_values"] = ch.dict_num_values;
  d["values"] = vec_to_tensor_u8(std::move(ch.values));
  d["validity"] = vec_to_tensor_u8(std::move(ch.validity));
  d["dict"] = vec_to_tensor_u8(std::move(ch.dict));
  // idx pages as int64 [n,5]
  auto pt = torch::empty({(int64_t)ch.idx_pages.size(), 5}, torch::kInt64);
  auto pa = pt.accessor<int64_t, 2>();
  for (size_t i = 0; i < ch.idx_pages.size(); i++) {
    pa[i][0] = ch.idx_pages[i].out_off;
    pa[i][1] = ch.idx_pages[i].n;
    pa[i][2] = ch.idx_pages[i].payload_off;
    pa[i][3] = ch.idx_pages[i].payload_len;
    pa[i][4] = ch.idx_pages[i].bit_width;
  }
  d["idx_pages"] = pt;
  return d;
}

static py::dict read_chunk_raw(int64_t h, int64_t rg, int64_t col) {
  auto f = get_file(h);
  ParquetFile::ChunkData ch;
  {
    py::gil_scoped_release rel;
    ch = f->read_chunk((size_t)rg, (size_t)col);
  }
  return chunk_to_dict_raw(std::move(ch));
}

static py::dict decoded_to_dict(DecodedColumn&& dc) {
  py::dict d;
  d["num_values"] = dc.num_values;
  d["data"] = vec_to_tensor_u8(std::move(dc.data));
  d["offsets"] = vec_to_tensor_i32(std::move(dc.offsets));
  d["bytes"] = vec_to_tensor_u8(std::move(dc.bytes));
  d["validity"] = vec_to_tensor_u8(std::move(dc.validity));
  if (dc.is_list) {
    auto lo = torch::empty({(int64_t)dc.list_offsets.size()}, torch::kInt64);
    std::memcpy(lo.data_ptr(), dc.list_offsets.data(),
                dc.list_offsets.size() * 8);
    d["list_offsets"] = lo;
    auto lv = torch::empty({(int64_t)dc.list_validity.size()}, torch::kUInt8);
    if (!dc.list_validity.empty())
      std::memcpy(lv.data_ptr(), dc.list_validity.data(),
                  dc.list_validity.size());
    d["list_validity"] = lv;
  }
  return d;
}

static py::dict read_chunk_cpu(int64_t h, int64_t rg, int64_t col) {
  auto f = get_file(h);
  DecodedColumn dc;
  torch::Tensor list_offs, list_valid;
  bool is_list = false;
  {
    py::gil_scoped_release rel;
    auto ch = f->read_chunk((size_t)rg, (size_t)col);
    if (ch.is_list) {
      is_list = true;
      list_offs = torch::empty({(int64_t)ch.list_offsets.size()}, torch::kInt64);
      std::memcpy(list_offs.data_ptr(), ch.list_offsets.data(),
                  ch.list_offsets.size() * 8);
      list_valid = torch::empty({(int64_t)ch.list_validity.size()}, torch::kUInt8);
      if (!ch.list_validity.empty())
        std::memcpy(list_valid.data_ptr(), ch.list_validity.data(),
                    ch.list_validity.size());
    }
    dc = decode_chunk_cpu(ch);
  }
  py::dict d = decoded_to_dict(std::move(dc));
  if (is_list) {
    d["list_offsets"] = list_offs;
    d["list_validity"] = list_valid;
  }
  return d;
}

// batch: parallel host decode across (rg,col) pairs
static py::list read_chunks_cpu_batch(int64_t h,
                                      const std::vector<std::pair<int64_t, int64_t>>& rc,
                                      int64_t nthreads) {
  auto f = get_file(h);
  std::vector<DecodedColumn> out(rc.size());
  {
    py::gil_scoped_release rel;
    std::string err;
    std::mutex err_mu;
    ThreadPool::instance().parallel_for((int64_t)rc.size(), [&](int64_t i) {
      try {
        auto ch = f->read_chunk((size_t)rc[i].first, (size_t)rc[i].second);
        out[i] = decode_chunk_cpu(ch);
      } catch (std::exception& e) {
        std::lock_guard<std::mutex> lk(err_mu);
        err = e.what();
      }
    });
    if (!err.empty()) throw std::runtime_error(err);
  }
  py::list result;
  for (auto& dc : out) result.append(decoded_to_dict(std::move(dc)));
  return result;
}

static py::list read_chunks_raw_batch(int64_t h,
                                      const std::vector<std::pair<int64_t, int64_t>>& rc,
                                      int64_t nthreads) {
  auto f = get_file(h);
  std::vector<ParquetFile::ChunkData> out(rc.size());
  {
    py::gil_scoped_release rel;
    std::string err;
    std::mutex err_mu;
    ThreadPool::instance().parallel_for((int64_t)rc.size(), [&](int64_t i) {
      try {
        out[i] = f->read_chunk((size_t)rc[i].first, (size_t)rc[i].second);
      } catch (std::exception& e) {
        std::lock_guard<std::mutex> lk(err_mu);
        err = e.what();
      }
    });
    if (!err.empty()) throw std::runtime_error(err);
  }
  py::list result;
  for (auto& ch : out) result.append(chunk_to_dict_raw(std::move(ch)));
  return result;
}

// read all files of a scan unit in one call; big contiguous buffers for
// single-H2D GPU decode (see read_unit.h). ``pin`` requests pinned host
// memory for the big buffers (GPU boxes).
static py::dict read_unit_raw_py(const std::vector<std::string>& paths,
                                 const std::vector<std::string>& names,
                                 int64_t nthreads, bool pin, bool gpu_snappy,
                                 bool gpu_zstd, double gpu_zstd_frac,
                                 bool gpu_delta, bool gpu_huf, bool gpu_lz4,
                                 bool gpu_strings, bool gpu_gzip) {
  (void)nthreads;
  std::unique_ptr<UnitStage> st;
  auto t0 = std::chrono::steady_clock::now();
  {
    py::gil_scoped_release rel;
    st = read_unit_stage1(paths, names, gpu_snappy, gpu_zstd, gpu_zstd_frac,
                          gpu_delta, gpu_huf, gpu_lz4, gpu_strings, gpu_gzip);
  }
  auto t1 = std::chrono::steady_clock::now();
  UnitStage& ud = *st;
  auto alloc_u8 = [&](int64_t n) {
    auto opts = torch::TensorOptions().dtype(torch::kUInt8);
    if (pin) {
      try {
        return torch::empty({n}, opts.pinned_memory(true));
      } catch (...) {
      }
    }
    return torch::empty({n}, opts);
  };
  torch::Tensor values = alloc_u8(ud.values_size);
  torch::Tensor validity = alloc_u8(ud.validity_size);
  torch::Tensor dicts = alloc_u8(ud.dicts_size);
  torch::Tensor soffs = torch::empty({ud.soffs_size}, torch::kInt64);
  torch::Tensor comp = alloc_u8(ud.comp_size);
  torch::Tensor runs = torch::empty({(int64_t)ud.runs.size()}, torch::kInt64);
  if (!ud.runs.empty())
    std::memcpy(runs.data_ptr(), ud.runs.data(), ud.runs.size() * 8);
  torch::Tensor enc = torch::empty({(int64_t)ud.enc.size()}, torch::kInt64);
  if (!ud.enc.empty())
    std::memcpy(enc.data_ptr(), ud.enc.data(), ud.enc.size() * 8);
  torch::Tensor sjobs = torch::empty({(int64_t)ud.snappy_jobs.size()}, torch::kInt64);
  if (!ud.snappy_jobs.empty())
    std::memcpy(sjobs.data_ptr(), ud.snappy_jobs.data(), ud.snappy_jobs.size() * 8);
  torch::Tensor zjobs = torch::empty({(int64_t)ud.zstd_jobs.size()}, torch::kInt64);
  if (!ud.zstd_jobs.empty())
    std::memcpy(zjobs.data_ptr(), ud.zstd_jobs.data(), ud.zstd_jobs.size() * 8);
  torch::Tensor hjobs = torch::empty({(int64_t)ud.huf_jobs.size()}, torch::kInt64);
  if (!ud.huf_jobs.empty())
    std::memcpy(hjobs.data_ptr(), ud.huf_jobs.data(), ud.huf_jobs.size() * 8);
  torch::Tensor ljobs = torch::empty({(int64_t)ud.lz4_jobs.size()}, torch::kInt64);
  if (!ud.lz4_jobs.empty())
    std::memcpy(ljobs.data_ptr(), ud.lz4_jobs.data(), ud.lz4_jobs.size() * 8);
  torch::Tensor gjobs = torch::empty({(int64_t)ud.gzip_jobs.size()}, torch::kInt64);
  if (!ud.gzip_jobs.empty())
    std::memcpy(gjobs.data_ptr(), ud.gzip_jobs.data(), ud.gzip_jobs.size() * 8);
  auto t2 = std::chrono::steady_clock::now();
  {
    py::gil_scoped_release rel;
    read_unit_fill(ud, (uint8_t*)values.data_ptr(), (uint8_t*)validity.data_ptr(),
                   (uint8_t*)dicts.data_ptr(), soffs.data_ptr<int64_t>(),
                   ud.comp_size ? (uint8_t*)comp.data_ptr() : nullptr);
  }
  auto t3 = std::chrono::steady_clock::now();
  py::dict d;
  auto us = [](auto a, auto b) {
    return std::chrono::duration_cast<std::chrono::microseconds>(b - a).count();
  };
  d["t_stage1_us"] = us(t0, t1);
  d["t_open_us"] = ud.t_open_us;
  d["t_chunks_us"] = ud.t_chunks_us;
  d["t_layout_us"] = ud.t_layout_us;
  d["t_alloc_us"] = us(t1, t2);
  d["t_fill_us"] = us(t2, t3);
  d["values"] = values;
  d["validity"] = validity;
  d["dicts"] = dicts;
  d["runs"] = runs;
  d["soffs"] = soffs;
  d["enc"] = enc;
  d["comp"] = comp;
  d["snappy_jobs"] = sjobs;
  d["zstd_jobs"] = zjobs;
  d["huf_jobs"] = hjobs;
  d["lz4_jobs"] = ljobs;
  d["gzip_jobs"] = gjobs;
  py::list frows;
  for (auto r : ud.file_rows) frows.append(r);
  d["file_rows"] = frows;
  // descriptor tensor for the GPU decoder (layout: unit_desc.h)
  auto dt = torch::empty({(int64_t)ud.cols.size(), UD_NFIELDS}, torch::kInt64);
  auto da = dt.accessor<int64_t, 2>();
  for (size_t i = 0; i < ud.cols.size(); i++) {
    const UnitColumn& c = ud.cols[i];
    da[i][UD_PRESENT] = c.present;
    da[i][UD_IS_STRING] = c.is_string;
    da[i][UD_IS_LIST] = c.is_list;
    da[i][UD_IS_DICT] = c.is_dict;
    da[i][UD_ESIZE] =
        c.present && !c.is_string ? physical_elem_size(c.physical) : 0;
    da[i][UD_NUM_VALUES] = c.num_values;
    da[i][UD_NULL_COUNT] = c.null_count;
    da[i][UD_VAL_OFF] = c.val_off;
    da[i][UD_VAL_LEN] = c.val_len;
    da[i][UD_VALIDITY_OFF] = c.validity_off;
    da[i][UD_DICT_OFF] = c.dict_off;
    da[i][UD_DICT_LEN] = c.dict_len;
    da[i][UD_RUN_OFF] = c.run_off;
    da[i][UD_RUN_CNT] = c.run_cnt;
    da[i][UD_DENSE_N] = c.dense_n;
    da[i][UD_SOFF_OFF] = c.soff_off;
    da[i][UD_SBYTES_OFF] = c.sbytes_off;
    da[i][UD_SBYTES_LEN] = c.sbytes_len;
    da[i][UD_ENC] = c.enc;
    da[i][UD_ENC_OFF] = c.enc_off;
    da[i][UD_ENC_CNT] = c.enc_cnt;
    da[i][UD_ENC_PAGES] = c.enc_pages;
    da[i][UD_STR] = c.str_kind;
  }
  d["desc"] = dt;
  // free the staging structures (dozens of MB of chunk vectors) off the
  // critical path — destructor cost was visible in the fetch time
  std::thread([p = st.release()]() { delete p; }).detach();
  return d;
}

// ---------------------------------------------------------------------- //
// murmur3 (CPU)
// ---------------------------------------------------------------------- //

// Hash fixed-width columns with seed chaining; returns int64 tensor of u32
// hashes. columns: CPU tensors (bool/int8/16/32/64/float32/64). Strings:
// pass (offsets,bytes) via hash_string_column step.
static torch::Tensor hash_columns_cpu(
    const std::vector<torch::Tensor>& columns,
    const std::vector<c10::optional<torch::Tensor>>& validity) {
  TORCH_CHECK(!columns.empty());
  int64_t n = columns[0].numel();
  auto out = torch::empty({n}, torch::kInt64);
  int64_t* hp = out.data_ptr<int64_t>();
  std::vector<torch::Tensor> cols;
  for (auto& c : columns) cols.push_back(c.contiguous().cpu());

  for (size_t ci = 0; ci < cols.size(); ci++) {
    torch::Tensor c = cols[ci];
    const uint8_t* vmask = nullptr;
    torch::Tensor vt;
    if (validity[ci].has_value()) {
      vt = validity[ci]->contiguous().cpu().to(torch::kUInt8);
      vmask = vt.data_ptr<uint8_t>();
    }
    auto st = c.scalar_type();
    at::parallel_for(0, n, 4096, [&](int64_t b, int64_t e) {
      for (int64_t i = b; i < e; i++) {
        uint32_t seed = ci == 0 ? kHashSeed : (uint32_t)hp[i];
        if (vmask && !vmask[i]) {
          if (ci == 0) hp[i] = 0;
          continue;
        }
        uint32_t hv;
        switch (st) {
          case torch::kBool:
            hv = spark_hash_u32((uint32_t)c.data_ptr<bool>()[i], seed);
            break;
          case torch::kInt8:
            hv = spark_hash_u32((uint32_t)(int32_t)c.data_ptr<int8_t>()[i], seed);
            break;
          case torch::kInt16:
            hv = spark_hash_u32((uint32_t)(int32_t)c.data_ptr<int16_t>()[i], seed);
            break;
          case torch::kInt32:
            hv = spark_hash_u32((uint32_t)c.data_ptr<int32_t>()[i], seed);
            break;
          case torch::kInt64:
            hv = spark_hash_u64((uint64_t)c.data_ptr<int64_t>()[i], seed);
            break;
          case torch::kFloat:
            hv = spark_hash_f32(c.data_ptr<float>()[i], seed);
            break;
          case torch::kDouble:
            hv = spark_hash_f64(c.data_ptr<double>()[i], seed);
            break;
          default:
            hv = 0;  // checked below
        }
        hp[i] = (int64_t)hv;
      }
    });
    TORCH_CHECK(st == torch::kBool || st == torch::kInt8 || st == torch::kInt16 ||
                    st == torch::kInt32 || st == torch::kInt64 ||
                    st == torch::kFloat || st == torch::kDouble,
                "unsupported dtype for murmur3");
  }
  return out;
}

// string column step: chain into existing hashes (or start, col_index==0)
static torch::Tensor hash_string_column_cpu(torch::Tensor offsets,
                                            torch::Tensor bytes,
                                            c10::optional<torch::Tensor> validity,
                                            c10::optional<torch::Tensor> prev,
                                            bool first_column) {
  auto off = offsets.contiguous().cpu().to(torch::kInt32);
  auto by = bytes.contiguous().cpu();
  int64_t n = off.numel() - 1;
  auto out = prev.has_value() ? prev->clone() : torch::zeros({n}, torch::kInt64);
  int64_t* hp = out.data_ptr<int64_t>();
  const int32_t* op = off.data_ptr<int32_t>();
  const uint8_t* bp = (const uint8_t*)by.data_ptr();
  const uint8_t* vmask = nullptr;
  torch::Tensor vt;
  if (validity.has_value()) {
    vt = validity->contiguous().cpu().to(torch::kUInt8);
    vmask = vt.data_ptr<uint8_t>();
  }
  at::parallel_for(0, n, 4096, [&](int64_t b, int64_t e) {
    for (int64_t i = b; i < e; i++) {
      if (vmask && !vmask[i]) {
        if (first_column) hp[i] = 0;
        continue;
      }
      uint32_t seed = first_column ? kHashSeed : (uint32_t)hp[i];
      hp[i] = (int64_t)spark_hash_bytes(bp + op[i], op[i + 1] - op[i], seed);
    }
  });
  return out;
}

static torch::Tensor bucket_ids_from_hashes(torch::Tensor hashes, int64_t nbuckets) {
  auto h = hashes.contiguous().cpu();
  int64_t n = h.numel();
  auto out = torch::empty({n}, torch::kInt32);
  const int64_t* hp = h.data_ptr<int64_t>();
  int32_t* op = out.data_ptr<int32_t>();
  for (int64_t i = 0; i < n; i++)
    op[i] = (int32_t)((uint32_t)hp[i] % (uint32_t)nbuckets);
  return out;
}

// list<string> columns ride the MOR merge as opaque per-row byte blobs
// whose payload is the PLAIN parquet representation ([u32 len][bytes]
// per element). After merge this parses the stream back into row ->
// element and element -> byte offsets (the chain walk is sequential, so
// it lives here at memcpy speed instead of a python loop).
static py::dict split_len_prefixed(const torch::Tensor& bytes,
                                   const torch::Tensor& row_byte_offsets) {
  torch::Tensor b = bytes.contiguous().cpu();
  torch::Tensor ro = row_byte_offsets.contiguous().cpu().to(torch::kInt64);
  const uint8_t* bp = b.data_ptr<uint8_t>();
  const int64_t* rp = ro.data_ptr<int64_t>();
  int64_t nrows = ro.numel() - 1;
  int64_t total = b.numel();
  // count elements first (u32 walk)
  int64_t m = 0;
  {
    int64_t p = 0;
    while (p + 4 <= total) {
      uint32_t len;
      std::memcpy(&len, bp + p, 4);
      p += 4 + len;
      m++;
    }
    TORCH_CHECK(p == total, "corrupt len-prefixed stream");
  }
  auto row_eoffs = torch::empty({nrows + 1}, torch::kInt64);
  auto eoffs = torch::empty({m + 1}, torch::kInt64);
  int64_t out_bytes = total - 4 * m;
  auto payload = torch::empty({out_bytes}, torch::kUInt8);
  int64_t* rep = row_eoffs.data_ptr<int64_t>();
  int64_t* ep = eoffs.data_ptr<int64_t>();
  uint8_t* pp = payload.data_ptr<uint8_t>();
  int64_t p = 0, e = 0, w = 0, r = 0;
  ep[0] = 0;
  rep[0] = 0;
  while (p + 4 <= total) {
    while (r < nrows && rp[r] == p) rep[r++] = e;  // rows ending here
    uint32_t len;
    std::memcpy(&len, bp + p, 4);
    p += 4;
    std::memcpy(pp + w, bp + p, len);
    p += len;
    w += len;
    ep[++e] = w;
  }
  while (r <= nrows) rep[r++] = e;  // trailing (incl. empty) rows
  py::dict d;
  d["row_offsets"] = row_eoffs;
  d["elem_offsets"] = eoffs;
  d["bytes"] = payload;
  return d;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "lakesoul_amd host-native core";
  m.def("write_parquet", &write_parquet, "write a parquet file",
        py::arg("path"), py::arg("names"), py::arg("dtypes"),
        py::arg("columns"), py::arg("offsets"), py::arg("validity"),
        py::arg("nullable"), py::arg("row_group_size"), py::arg("codec"),
        py::arg("level"),
        py::arg("elem_offsets") = std::vector<c10::optional<torch::Tensor>>{},
        py::arg("parents") = std::vector<std::string>{});
  m.def("writer_open", &writer_open, py::arg("path"), py::arg("names"),
        py::arg("dtypes"), py::arg("nullable"), py::arg("row_group_size"),
        py::arg("codec"), py::arg("level"),
        py::arg("parents") = std::vector<std::string>{});
  m.def("writer_write", &writer_write, py::arg("h"), py::arg("columns"),
        py::arg("offsets"), py::arg("validity"),
        py::arg("elem_offsets") = std::vector<c10::optional<torch::Tensor>>{});
  m.def("split_len_prefixed", &split_len_prefixed,
        "parse a PLAIN len-prefixed byte-array stream back into row/element offsets");
  m.def("writer_bytes", &writer_bytes);
  m.def("writer_finish", &writer_finish);
  m.def("writer_abort", &writer_abort);
  m.def("open_parquet", &open_parquet);
  m.def("close_parquet", &close_parquet);
  m.def("parquet_meta", &parquet_meta);
  m.def("read_chunk_raw", &read_chunk_raw);
  m.def("read_chunk_cpu", &read_chunk_cpu);
  m.def("read_chunks_cpu_batch", &read_chunks_cpu_batch);
  m.def("read_unit_raw", &read_unit_raw_py, py::arg("paths"), py::arg("names"),
        py::arg("nthreads") = 0, py::arg("pin") = true,
        py::arg("gpu_snappy") = false, py::arg("gpu_zstd") = false,
        py::arg("gpu_zstd_frac") = 1.0, py::arg("gpu_delta") = false,
        py::arg("gpu_huf") = false, py::arg("gpu_lz4") = false,
        py::arg("gpu_strings") = false, py::arg("gpu_gzip") = false);
  // the one descriptor column python looks at (fast-path eligibility)
  m.attr("UD_PRESENT") = (int)UD_PRESENT;
  // where a column's regions lie, and its GPU-decoded value encoding
  // (tests read both off the descriptor)
  m.attr("UD_NUM_VALUES") = (int)UD_NUM_VALUES;
  m.attr("UD_NULL_COUNT") = (int)UD_NULL_COUNT;
  m.attr("UD_VAL_OFF") = (int)UD_VAL_OFF;
  m.attr("UD_VAL_LEN") = (int)UD_VAL_LEN;
  m.attr("UD_VALIDITY_OFF") = (int)UD_VALIDITY_OFF;
  m.attr("UD_SOFF_OFF") = (int)UD_SOFF_OFF;
  m.attr("UD_SBYTES_OFF") = (int)UD_SBYTES_OFF;
  m.attr("UD_SBYTES_LEN") = (int)UD_SBYTES_LEN;
  m.attr("UD_ENC") = (int)UD_ENC;
  m.attr("UD_ENC_OFF") = (int)UD_ENC_OFF;
  m.attr("UD_ENC_CNT") = (int)UD_ENC_CNT;
  m.attr("UD_ENC_PAGES") = (int)UD_ENC_PAGES;
  m.attr("UD_IS_DICT") = (int)UD_IS_DICT;
  m.attr("UD_DICT_OFF") = (int)UD_DICT_OFF;
  m.attr("UD_DICT_LEN") = (int)UD_DICT_LEN;
  m.attr("UD_RUN_OFF") = (int)UD_RUN_OFF;
  m.attr("UD_RUN_CNT") = (int)UD_RUN_CNT;
  m.attr("UD_DENSE_N") = (int)UD_DENSE_N;
  m.attr("UD_STR") = (int)UD_STR;
  m.attr("UD_STR_PLAIN") = (int)UD_STR_PLAIN;
  m.attr("UD_STR_DICT") = (int)UD_STR_DICT;
  m.attr("UD_ENC_DELTA_BINARY") = (int)ParquetFile::ENCK_DELTA_BINARY;
  m.attr("UD_ENC_BYTE_STREAM_SPLIT") = (int)ParquetFile::ENCK_BYTE_STREAM_SPLIT;
  m.def("read_chunks_raw_batch", &read_chunks_raw_batch);
  // GPU string route: the host twins of _hip.strip_prefixes / dict_strings
  // (str_seg.h) and the two prefix walks (str_walk.h)
  m.def("strip_prefixes", [](torch::Tensor raw, torch::Tensor doff) {
    TORCH_CHECK(raw.is_cpu() && raw.scalar_type() == torch::kUInt8 &&
                    raw.dim() == 1 && raw.is_contiguous() && doff.is_cpu() &&
                    doff.scalar_type() == torch::kInt64 && doff.dim() == 1 &&
                    doff.is_contiguous(),
                "strip_prefixes: raw uint8 and dense offsets int64, 1-d, on the host");
    int64_t n = doff.numel() ? doff.numel() - 1 : 0;
    auto out = lsseg::strip_prefixes_host(
        raw.numel() ? raw.data_ptr<uint8_t>() : nullptr, raw.numel(),
        doff.numel() ? doff.data_ptr<int64_t>() : nullptr, n);
    return vec_to_tensor_u8(std::move(out));
  });
  m.def("dict_strings", [](torch::Tensor idx, torch::Tensor dict_off,
                           torch::Tensor dict_bytes,
                           c10::optional<torch::Tensor> validity) {
    TORCH_CHECK(idx.is_cpu() && idx.scalar_type() == torch::kInt32 &&
                    idx.is_contiguous() && dict_off.is_cpu() &&
                    dict_off.scalar_type() == torch::kInt64 &&
                    dict_off.is_contiguous() && dict_off.numel() >= 1 &&
                    dict_bytes.is_cpu() &&
                    dict_bytes.scalar_type() == torch::kUInt8 &&
                    dict_bytes.is_contiguous(),
                "dict_strings: idx int32, dict_offsets int64 (entries + 1), "
                "dict_bytes uint8, on the host");
    const uint8_t* vp = nullptr;
    int64_t nrows = idx.numel();
    if (validity.has_value()) {
      TORCH_CHECK(validity->is_cpu() && validity->scalar_type() == torch::kUInt8 &&
                      validity->is_contiguous(),
                  "dict_strings: validity uint8 on the host");
      nrows = validity->numel();
      vp = nrows ? validity->data_ptr<uint8_t>() : nullptr;
      if (!vp) validity.reset();
    }
    std::vector<int64_t> offs;
    std::vector<uint8_t> bytes;
    int32_t st = lsseg::dict_strings_host(
        idx.numel() ? idx.data_ptr<int32_t>() : nullptr, idx.numel(),
        dict_off.data_ptr<int64_t>(), dict_off.numel() - 1,
        dict_bytes.numel() ? dict_bytes.data_ptr<uint8_t>() : nullptr,
        dict_bytes.numel(), vp, nrows, offs, bytes);
    auto ot = torch::empty({(int64_t)offs.size()}, torch::kInt64);
    std::memcpy(ot.data_ptr(), offs.data(), offs.size() * 8);
    auto stt = torch::full({1}, (int64_t)st, torch::kInt32);
    return py::make_tuple(ot, vec_to_tensor_u8(std::move(bytes)), stt);
  }, py::arg("idx"), py::arg("dict_offsets"), py::arg("dict_bytes"),
     py::arg("validity") = py::none());
  m.def("str_walk_plain", [](py::bytes src, int64_t expect) {
    std::string b = src;
    std::unique_ptr<uint8_t[]> in(new uint8_t[b.size() ? b.size() : 1]);
    std::memcpy(in.get(), b.data(), b.size());
    std::vector<int64_t> offs{0};
    int64_t total = 0;
    str_walk_plain(in.get(), b.size(), expect, total, offs);
    auto ot = torch::empty({(int64_t)offs.size()}, torch::kInt64);
    std::memcpy(ot.data_ptr(), offs.data(), offs.size() * 8);
    return ot;
  });
  m.def("str_walk_dict", [](py::bytes src, int64_t nent) {
    std::string b = src;
    std::unique_ptr<uint8_t[]> in(new uint8_t[b.size() ? b.size() : 1]);
    std::memcpy(in.get(), b.data(), b.size());
    std::vector<int64_t> offs{0};
    std::vector<uint8_t> bytes;
    int64_t total = 0;
    str_walk_dict(in.get(), b.size(), nent, total, offs, bytes);
    auto ot = torch::empty({(int64_t)offs.size()}, torch::kInt64);
    std::memcpy(ot.data_ptr(), offs.data(), offs.size() * 8);
    return py::make_tuple(ot, vec_to_tensor_u8(std::move(bytes)));
  });
  m.def("zstd_compress_ref", [](py::bytes src, int64_t level) {
    std::string b = src;
    auto out = zstd_compress((const uint8_t*)b.data(), b.size(), (int)level);
    return py::bytes((const char*)out.data(), out.size());
  });
  m.def("zstd_decompress_ref", [](py::bytes src, int64_t cap) {
    std::string b = src;
    std::vector<uint8_t> out((size_t)cap);
    zstd_decompress_into(out.data(), (size_t)cap, (const uint8_t*)b.data(),
                         b.size());
    return py::bytes((const char*)out.data(), (size_t)cap);
  });
  m.def("zstd_decode_ref", [](py::bytes src, int64_t cap) {
    // differential-test hook for the from-scratch zstd decoder
    std::string b = src;
    std::vector<uint8_t> out((size_t)cap);
    static thread_local std::unique_ptr<lszstd::Ctx> ctx;
    if (!ctx) ctx.reset(new lszstd::Ctx());
    int64_t n = lszstd::decode((const uint8_t*)b.data(), (int64_t)b.size(),
                               out.data(), cap, ctx.get());
    if (n < 0) throw std::runtime_error("lszstd decode failed");
    return py::bytes((const char*)out.data(), (size_t)n);
  });
  // the LZ4 block codec (lz4_dec.h): decoder hooks return None for a block
  // they refuse
  m.def("lz4_block_decode_ref", [](py::bytes src, int64_t n) -> py::object {
    std::string b = src;
    if (n < 0) throw std::runtime_error("lz4_block_decode_ref: n < 0");
    std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)n ? (size_t)n : 1]);
    if (!lslz4::lz4_block_decode(out.get(), n, (const uint8_t*)b.data(),
                                 (int64_t)b.size()))
      return py::none();
    return py::bytes((const char*)out.get(), (size_t)n);
  });
  m.def("lz4_hadoop_decode_ref", [](py::bytes src, int64_t n) -> py::object {
    std::string b = src;
    if (n < 0) throw std::runtime_error("lz4_hadoop_decode_ref: n < 0");
    std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)n ? (size_t)n : 1]);
    if (!lslz4::lz4_hadoop_decode(out.get(), n, (const uint8_t*)b.data(),
                                  (int64_t)b.size()))
      return py::none();
    return py::bytes((const char*)out.get(), (size_t)n);
  });
  // DEFLATE (inflate.h): a parquet GZIP page (gzip members or a zlib
  // stream) and a bare DEFLATE stream; None for input they refuse
  m.def("inflate_ref", [](py::bytes src, int64_t n) -> py::object {
    std::string b = src;
    if (n < 0) throw std::runtime_error("inflate_ref: n < 0");
    std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)n ? (size_t)n : 1]);
    if (!lsinfl::inflate_page(out.get(), n, (const uint8_t*)b.data(),
                              (int64_t)b.size()))
      return py::none();
    return py::bytes((const char*)out.get(), (size_t)n);
  });
  m.def("inflate_raw_ref", [](py::bytes src, int64_t n) -> py::object {
    std::string b = src;
    if (n < 0) throw std::runtime_error("inflate_raw_ref: n < 0");
    std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)n ? (size_t)n : 1]);
    if (!lsinfl::inflate_raw(out.get(), n, (const uint8_t*)b.data(),
                             (int64_t)b.size()))
      return py::none();
    return py::bytes((const char*)out.get(), (size_t)n);
  });
  m.def("lz4_compress_ref", [](py::bytes src) {
    std::string b = src;
    auto out = lz4_compress((const uint8_t*)b.data(), b.size());
    return py::bytes((const char*)out.data(), out.size());
  });
  m.def("zstd_frame_census", [](py::bytes bytes) {
    // what format features the frames in `bytes` use: walks them with the
    // decoder's parse functions only, decodes nothing
    using namespace lszstd;
    std::string buf = bytes;
    const uint8_t* src = (const uint8_t*)buf.data();
    const int64_t n = (int64_t)buf.size();
    std::map<std::string, int64_t> count;
    auto fail = [] { throw std::runtime_error("zstd_frame_census: bad frame"); };
    static const char* const kBlock[] = {"raw", "rle", "compressed"};
    static const char* const kLit[] = {"raw", "rle", "compressed", "treeless"};
    static const char* const kTable[] = {"ll", "of", "ml"};
    int64_t ip = 0;
    while (ip + 4 <= n) {
      bool skippable, checksum;
      ip = parse_frame_header(src, n, ip, skippable, checksum);
      if (ip < 0) fail();
      if (skippable) continue;
      BlockHdr b;
      do {
        if (!parse_block_header(src + ip, n - ip, b)) fail();
        ip += 3;
        count[std::string("block_") + kBlock[b.type]]++;
        if (b.type == kBlockCompressed) {
          const uint8_t* p = src + ip;
          LitHdr h;
          if (!parse_literals_header(p, b.size, h)) fail();
          // header form: its length for raw / RLE, the size format otherwise
          int form = h.type <= kLitRle ? (int)h.hdr : h.sizeFormat;
          count[std::string("lit_") + kLit[h.type] + "_" + std::to_string(form)]++;
          if (h.type == kLitCompressed && h.cs >= 1)
            count[huf_desc_direct(p[h.hdr]) ? "huf_direct" : "huf_fse"]++;
          p += h.hdr + h.cs;
          int64_t rem = b.size - (h.hdr + h.cs), nSeq;
          int used = read_seq_count(p, rem, nSeq);
          if (used < 0 || (nSeq > 0 && rem < used + 1)) fail();
          count["nseq_" + std::to_string(used) + "byte"]++;
          if (nSeq == 0) count["nseq_zero"]++;
          for (int kind = kSeqLL; nSeq > 0 && kind <= kSeqML; kind++)
            count[std::string(kTable[kind]) + "_mode_" +
                  std::to_string(seq_mode(p[used], kind))]++;
        }
        ip += b.srcBytes;
      } while (!b.last);
      if (checksum) ip += 4;
    }
    return count;
  });
  m.def("zstd_huf_only", [](py::bytes bytes, int64_t rs) {
    // the page classifier of the GPU Huffman route: is `bytes` a
    // Huffman-only page of rs bytes?
    std::string b = bytes;
    lszstd::HufOnly ho;
    const uint8_t* src = (const uint8_t*)b.data();
    return lszstd::huf_only_frame(src, (int64_t)b.size(), rs, ho);
  }, py::arg("frame"), py::arg("rs"));
  m.def("zstd_huf_census", [](py::bytes bytes, int64_t rs) {
    // of an accepted frame: streams, literals size format, the table's
    // maxBits and whether the tree description is direct or FSE-compressed
    std::string b = bytes;
    const uint8_t* src = (const uint8_t*)b.data();
    lszstd::HufOnly ho;
    if (!lszstd::huf_only_frame(src, (int64_t)b.size(), rs, ho))
      throw std::runtime_error("zstd_huf_census: not a Huffman-only frame");
    auto c = std::make_unique<lszstd::HufParCtx>();
    if (lszstd::read_huf_tree(src + ho.payload, ho.cs, c->huf, c->ws) < 0)
      throw std::runtime_error("zstd_huf_census: bad tree description");
    py::dict d;
    d["streams"] = ho.nStreams;
    d["size_format"] = ho.sizeFormat;
    d["rs"] = ho.rs;
    d["max_bits"] = c->huf.maxBits;
    d["tree"] = lszstd::huf_desc_direct(src[ho.payload]) ? "direct" : "fse";
    return d;
  });
  m.def("zstd_huf_par_decode_ref", [](py::bytes bytes, int64_t lanes, int64_t rs) {
    // host twin of the GPU Huffman kernel (csrc/cpp/huf_par.h). Returns
    // (bytes, fix-up rounds), or (None, rounds) where the decode fails;
    // the destination is exactly rs bytes on the heap.
    std::string b = bytes;
    const uint8_t* src = (const uint8_t*)b.data();
    if (rs < 0) throw std::runtime_error("zstd_huf_par_decode_ref: rs < 0");
    auto c = std::make_unique<lszstd::HufParCtx>();
    std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)rs]);
    bool ok = lszstd::huf_par_decode(src, (int64_t)b.size(), out.get(), rs,
                                     (int)lanes, *c);
    if (!ok) return py::make_tuple(py::none(), c->rounds);
    return py::make_tuple(py::bytes((const char*)out.get(), (size_t)rs), c->rounds);
  }, py::arg("frame"), py::arg("lanes"), py::arg("rs"));
  // string predicates (str_pred.h): the operand compilers and the host twin
  // of the GPU kernel. An operand is (bytes uint8, meta int32).
  m.def("str_pred_compile_literal", [](py::bytes lit) {
    std::string b = lit;
    std::vector<uint8_t> bytes;
    std::vector<int32_t> meta;
    lspred::compile_literal((const uint8_t*)b.data(), (int64_t)b.size(), bytes, meta);
    return py::make_tuple(torch::tensor(bytes, torch::kUInt8),
                          torch::tensor(meta, torch::kInt32));
  }, py::arg("literal"));
  m.def("str_pred_compile_set", [](std::vector<py::bytes> lits) {
    std::vector<std::string> v;
    for (auto& l : lits) v.push_back((std::string)l);
    std::vector<uint8_t> bytes;
    std::vector<int32_t> meta;
    lspred::compile_set(std::move(v), bytes, meta);
    return py::make_tuple(torch::tensor(bytes, torch::kUInt8),
                          torch::tensor(meta, torch::kInt32));
  }, py::arg("literals"));
  m.def("str_pred_compile_like", [](py::bytes pattern, int64_t escape, bool utf8) {
    std::string b = pattern;
    std::vector<uint8_t> bytes;
    std::vector<int32_t> meta;
    lspred::compile_like((const uint8_t*)b.data(), (int64_t)b.size(),
                         escape < 0 || escape > 255 ? -1 : (int)escape, utf8,
                         bytes, meta);
    return py::make_tuple(torch::tensor(bytes, torch::kUInt8),
                          torch::tensor(meta, torch::kInt32));
  }, py::arg("pattern"), py::arg("escape"), py::arg("utf8"));
  m.def("str_pred_mask", [](torch::Tensor offsets, torch::Tensor bytes,
                            c10::optional<torch::Tensor> validity, int64_t op,
                            torch::Tensor op_bytes, torch::Tensor op_meta) {
    TORCH_CHECK(!offsets.is_cuda() && !bytes.is_cuda() && !op_bytes.is_cuda() &&
                !op_meta.is_cuda(), "str_pred_mask: CPU tensors only");
    TORCH_CHECK(op >= 0 && op < lspred::OP_COUNT, "str_pred_mask: bad op");
    TORCH_CHECK(offsets.dim() == 1 && offsets.numel() >= 1, "str_pred_mask: offsets");
    TORCH_CHECK(bytes.scalar_type() == torch::kUInt8 &&
                op_bytes.scalar_type() == torch::kUInt8 &&
                op_meta.scalar_type() == torch::kInt32, "str_pred_mask: dtypes");
    offsets = offsets.contiguous();
    bytes = bytes.contiguous();
    op_bytes = op_bytes.contiguous();
    op_meta = op_meta.contiguous();
    TORCH_CHECK(op_meta.numel() >= lspred::min_meta((int)op), "str_pred_mask: short operand");
    int64_t n = offsets.numel() - 1;
    torch::Tensor val;
    const uint8_t* vp = nullptr;
    if (validity && validity->numel()) {
      TORCH_CHECK(validity->numel() == n && (validity->scalar_type() == torch::kUInt8 ||
                                             validity->scalar_type() == torch::kBool),
                  "str_pred_mask: validity");
      val = validity->contiguous();
      vp = (const uint8_t*)val.data_ptr();
    }
    auto out = torch::empty({n}, torch::kBool);
    lspred::Operand o{op_bytes.numel() ? op_bytes.data_ptr<uint8_t>() : nullptr,
                      op_bytes.numel(), op_meta.data_ptr<int32_t>(), op_meta.numel()};
    const uint8_t* bp = bytes.numel() ? bytes.data_ptr<uint8_t>() : nullptr;
    if (offsets.scalar_type() == torch::kInt32)
      lspred::str_pred_mask_host(offsets.data_ptr<int32_t>(), n, bp, bytes.numel(),
                                 vp, (int)op, o, (uint8_t*)out.data_ptr());
    else if (offsets.scalar_type() == torch::kInt64)
      lspred::str_pred_mask_host(offsets.data_ptr<int64_t>(), n, bp, bytes.numel(),
                                 vp, (int)op, o, (uint8_t*)out.data_ptr());
    else
      TORCH_CHECK(false, "str_pred_mask: offsets must be int32 or int64");
    return out;
  }, py::arg("offsets"), py::arg("bytes"), py::arg("validity"), py::arg("op"),
     py::arg("op_bytes"), py::arg("op_meta"));
  m.def("hash_columns_cpu", &hash_columns_cpu);
  m.def("hash_string_column_cpu", &hash_string_column_cpu);
  m.def("bucket_ids_from_hashes", &bucket_ids_from_hashes);
  m.def("spark_hash_bytes", [](py::bytes b, int64_t seed) {
    std::string s = b;
    return (int64_t)spark_hash_bytes((const uint8_t*)s.data(), (int64_t)s.size(),
                                     (uint32_t)seed);
  });
  // the batched-merge plan (merge_plan.h) of streams of these lengths, for
  // tests: (rounds, nbufs, n, tile_rows). A round is
  // (pairs, carry_or_None, buf_out, ntiles), a pair (a, b, first_tile,
  // ntiles), a stream (buf, first, count, off, n).
  m.def("merge_plan", [](std::vector<int64_t> lens) {
    auto st = [](const MergeStream& s) {
      return py::make_tuple(s.buf, s.first, s.count, s.off, s.n);
    };
    MergePlan plan = plan_merge(lens);
    py::list rounds;
    for (auto& r : plan.rounds) {
      py::list pairs;
      for (auto& p : r.pairs)
        pairs.append(py::make_tuple(st(p.a), st(p.b), p.first_tile, p.ntiles));
      rounds.append(py::make_tuple(pairs, r.has_carry ? py::object(st(r.carry)) : py::none(),
                                   r.buf_out, r.ntiles));
    }
    return py::make_tuple(rounds, plan.nbufs, plan.n, MERGE_TILE_ROWS);
  }, py::arg("lens"));
}
