// lakesoul_amd._hip — torch bindings for the gfx950 kernels (kernels.hip).
#include <torch/extension.h>

#include <hip/hip_runtime.h>

#include <c10/hip/HIPStream.h>

#include <atomic>

#include "../cpp/merge_plan.h"
#include "../cpp/str_pred.h"
#include "../cpp/unit_desc.h"
#include "kernels.h"

namespace py = pybind11;

using namespace lakesoul;

static hipStream_t cur_stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

#define CHECK_GPU(t) TORCH_CHECK((t).is_cuda(), #t " must be on GPU"); \
  TORCH_CHECK((t).is_contiguous(), #t " must be contiguous")

// optional/empty tensors may be placeholder CPU empties; any tensor the
// kernel will actually dereference must be device-resident (a CPU
// pointer reaching a kernel = memory fault, see Column.take fix)
#define CHECK_GPU_NONEMPTY(t)                                   \
  if ((t).numel()) {                                            \
    TORCH_CHECK((t).is_cuda(), #t " must be on GPU");           \
    TORCH_CHECK((t).is_contiguous(), #t " must be contiguous"); \
  }

static const uint8_t* opt_u8(const torch::Tensor& t) {
  return t.numel() ? t.data_ptr<uint8_t>() : nullptr;
}

// ---- hashing ---------------------------------------------------------- //

static torch::Tensor hash_fixed_column(torch::Tensor data, torch::Tensor validity,
                                       torch::Tensor prev, bool first) {
  CHECK_GPU_NONEMPTY(validity);
  CHECK_GPU_NONEMPTY(prev);
  CHECK_GPU(data);
  int64_t n = data.numel();
  auto out = torch::empty({n}, data.options().dtype(torch::kInt64));
  int dt;
  switch (data.scalar_type()) {
    case torch::kUInt8:
    case torch::kBool: dt = 0; break;
    case torch::kInt8: dt = 1; break;
    case torch::kInt16: dt = 2; break;
    case torch::kInt32: dt = 3; break;
    case torch::kInt64: dt = 4; break;
    case torch::kFloat: dt = 5; break;
    case torch::kDouble: dt = 6; break;
    default: TORCH_CHECK(false, "unsupported dtype for hash");
  }
  launch_hash_fixed(dt, data.data_ptr(), opt_u8(validity),
                    first ? nullptr : prev.data_ptr<int64_t>(),
                    out.data_ptr<int64_t>(), n, first ? 1 : 0, cur_stream());
  return out;
}

static torch::Tensor hash_string_column(torch::Tensor offsets, torch::Tensor bytes,
                                        torch::Tensor validity, torch::Tensor prev,
                                        bool first) {
  CHECK_GPU_NONEMPTY(bytes);
  CHECK_GPU_NONEMPTY(validity);
  CHECK_GPU_NONEMPTY(prev);
  CHECK_GPU(offsets);
  int64_t n = offsets.numel() - 1;
  auto out = torch::empty({n}, offsets.options().dtype(torch::kInt64));
  launch_hash_string(offsets.data_ptr<int32_t>(), bytes.data_ptr<uint8_t>(),
                     opt_u8(validity), first ? nullptr : prev.data_ptr<int64_t>(),
                     out.data_ptr<int64_t>(), n, first ? 1 : 0, cur_stream());
  return out;
}

static torch::Tensor bucket_ids(torch::Tensor hashes, int64_t nbuckets) {
  CHECK_GPU(hashes);
  int64_t n = hashes.numel();
  auto out = torch::empty({n}, hashes.options().dtype(torch::kInt32));
  launch_bucket_ids(hashes.data_ptr<int64_t>(), out.data_ptr<int32_t>(), n,
                    (uint32_t)nbuckets, cur_stream());
  return out;
}

// ---- decode ----------------------------------------------------------- //

// element-size dispatch for decode_unit_cols
static void dict_gather_scatter_es(int64_t es, const void* dict_vals,
                                   const int32_t* idx, const uint8_t* vmask,
                                   const int64_t* pos, void* out, int64_t n,
                                   hipStream_t stream) {
  if (es == 4)
    launch_dict_gather_scatter<uint32_t>((const uint32_t*)dict_vals, idx, vmask, pos, (uint32_t*)out, n, stream);
  else if (es == 8)
    launch_dict_gather_scatter<uint64_t>((const uint64_t*)dict_vals, idx, vmask, pos, (uint64_t*)out, n, stream);
  else if (es == 1)
    launch_dict_gather_scatter<uint8_t>((const uint8_t*)dict_vals, idx, vmask, pos, (uint8_t*)out, n, stream);
  else
    TORCH_CHECK(false, "dict_gather_scatter: unsupported elem size ", es);
}

static void scatter_valid_es(int64_t es, const void* dense, const uint8_t* vmask,
                             const int64_t* pos, void* out, int64_t n,
                             hipStream_t stream) {
  if (es == 1)
    launch_scatter_valid<uint8_t>((const uint8_t*)dense, vmask, pos, (uint8_t*)out, n, stream);
  else if (es == 2)
    launch_scatter_valid<uint16_t>((const uint16_t*)dense, vmask, pos, (uint16_t*)out, n, stream);
  else if (es == 4)
    launch_scatter_valid<uint32_t>((const uint32_t*)dense, vmask, pos, (uint32_t*)out, n, stream);
  else if (es == 8)
    launch_scatter_valid<uint64_t>((const uint64_t*)dense, vmask, pos, (uint64_t*)out, n, stream);
  else
    TORCH_CHECK(false, "scatter_valid: unsupported elem size ", es);
}

// ---- merge ------------------------------------------------------------ //

// K sorted key streams through the batched merge rounds (merge_plan.h,
// kernels.hip merge_round_kernel): one launch per round and 16 pairs, an
// odd stream carried forward by pointer; on equal keys the earlier (older)
// stream comes first. Input streams are int64 or int32 keys (key_format:
// MERGE_KEY_I64 / _I32, packed in registers) or already packed u64 keys in
// int64 storage (MERGE_KEY_PACKED). Row values are positions in the
// concatenation of the streams in input order; those of the inputs are
// computed, never stored.
//   keep_last = false: (merged packed keys, row of each merged key)
//   keep_last = true: (undefined, the row of the LAST of every run of equal
//     keys, in key order). The last round writes no keys and compacts the
//     survivors tile by tile; one host sync, at their total.
static std::pair<torch::Tensor, torch::Tensor> merge_rounds(
    const std::vector<torch::Tensor>& keys, int key_format, bool keep_last) {
  auto stream = cur_stream();
  auto i64 = keys[0].options().dtype(torch::kInt64);
  std::vector<int64_t> lens;
  for (auto& k : keys) lens.push_back(k.numel());
  MergePlan plan = plan_merge(lens);
  const int64_t n = plan.n;
  if (keep_last && plan.rounds.empty()) {
    // one stream: the keep-last round alone, against an empty B
    MergeRound r;
    MergePair p;
    p.a.n = n;
    p.b.off = n;
    p.ntiles = (n + MERGE_TILE_ROWS - 1) / MERGE_TILE_ROWS;
    r.pairs.push_back(p);
    r.buf_out = MP_RESULT;
    r.ntiles = p.ntiles;
    plan.rounds.push_back(r);
  }
  torch::Tensor out_keys, out_rows, kbuf, rbuf, counts;
  if (plan.nbufs) {
    kbuf = torch::empty({plan.nbufs, n}, i64);
    rbuf = torch::empty({plan.nbufs, n}, i64);
  }
  const int64_t last_tiles = plan.rounds.back().ntiles;
  if (keep_last) {
    out_rows = torch::empty({last_tiles * MERGE_TILE_ROWS}, i64);  // tile slots
    counts = torch::empty({last_tiles}, i64);
  } else {
    out_keys = torch::empty({n}, i64);
    out_rows = torch::empty({n}, i64);
  }
  auto set_stream = [&](const MergeStream& s, const void*& k, const int64_t*& r,
                        int64_t& cnt, int64_t& base) {
    cnt = s.n;
    base = s.off;
    if (s.buf == MP_INPUT) {
      k = s.n ? keys[(size_t)s.first].data_ptr() : nullptr;
      r = nullptr;
    } else {
      k = kbuf.data_ptr<int64_t>() + s.buf * n + s.off;
      r = rbuf.data_ptr<int64_t>() + s.buf * n + s.off;
    }
  };
  for (auto& round : plan.rounds) {
    const bool last = round.buf_out == MP_RESULT;
    for (size_t c0 = 0; c0 < round.pairs.size(); c0 += MERGE_PAIRS_PER_LAUNCH) {
      MergeTable tbl;
      tbl.npairs = 0;
      tbl.ntiles = 0;
      tbl.tile_counts = last && keep_last ? counts.data_ptr<int64_t>() : nullptr;
      for (size_t j = c0; j < round.pairs.size() && tbl.npairs < MERGE_PAIRS_PER_LAUNCH; j++) {
        const MergePair& p = round.pairs[j];
        MergePairArg& a = tbl.p[tbl.npairs++];
        set_stream(p.a, a.kA, a.rA, a.nA, a.baseA);
        set_stream(p.b, a.kB, a.rB, a.nB, a.baseB);
        if (last) {
          a.kOut = keep_last ? nullptr : (uint64_t*)out_keys.data_ptr<int64_t>() + p.a.off;
          a.rOut = out_rows.data_ptr<int64_t>() + p.a.off;
        } else {
          a.kOut = (uint64_t*)kbuf.data_ptr<int64_t>() + round.buf_out * n + p.a.off;
          a.rOut = rbuf.data_ptr<int64_t>() + round.buf_out * n + p.a.off;
        }
        a.first_tile = tbl.ntiles;
        tbl.ntiles += p.ntiles;
      }
      if (last && keep_last)
        launch_merge_round_keep_last(tbl, key_format, stream);
      else
        launch_merge_round(tbl, key_format, stream);
    }
  }
  if (!keep_last) return {out_keys, out_rows};
  if (last_tiles == 0) return {out_keys, torch::empty({0}, i64)};
  auto csum = at::cumsum(counts, 0);
  int64_t kept = csum[last_tiles - 1].item<int64_t>();  // the path's one sync
  auto src_idx = torch::empty({kept}, i64);
  launch_compact_tiles(out_rows.data_ptr<int64_t>(), counts.data_ptr<int64_t>(),
                       csum.data_ptr<int64_t>(), last_tiles,
                       src_idx.data_ptr<int64_t>(), stream);
  return {out_keys, src_idx};
}

// K sorted streams of packed u64 keys (int64 storage) -> (keys, order):
// the merged keys and, per merged row, its index in the concatenation of
// the streams in input order (the merge_sorted_keys binding).
static std::pair<torch::Tensor, torch::Tensor> merge_key_streams(
    std::vector<torch::Tensor> keys) {
  TORCH_CHECK(!keys.empty(), "merge_sorted_keys: no streams");
  for (auto& k : keys) {
    CHECK_GPU(k);
    TORCH_CHECK(k.scalar_type() == torch::kInt64 && k.dim() == 1,
                "merge_sorted_keys: keys must be 1-d int64");
  }
  if (keys.size() == 1)
    return {keys[0], torch::arange(keys[0].numel(), keys[0].options())};
  return merge_rounds(keys, MERGE_KEY_PACKED, false);
}

// K sorted streams of raw int64 or int32 keys -> src_idx: for every
// distinct key, in key order, the position of its LAST row in the
// concatenation of the streams in input order (later stream wins, inside a
// stream the later row). The merge of scan_unit_uselast; also the
// unit_merge_src_idx binding.
static torch::Tensor unit_merge_src_idx(std::vector<torch::Tensor> keys) {
  TORCH_CHECK(!keys.empty(), "unit_merge_src_idx: no streams");
  auto dt = keys[0].scalar_type();
  TORCH_CHECK(dt == torch::kInt64 || dt == torch::kInt32,
              "unit_merge_src_idx: keys must be int64 or int32");
  for (auto& k : keys) {
    CHECK_GPU(k);
    TORCH_CHECK(k.scalar_type() == dt && k.dim() == 1,
                "unit_merge_src_idx: keys must be 1-d and of one dtype");
  }
  return merge_rounds(keys, dt == torch::kInt64 ? MERGE_KEY_I64 : MERGE_KEY_I32, true)
      .second;
}

static torch::Tensor group_start_mask(torch::Tensor keys) {
  CHECK_GPU(keys);
  int64_t n = keys.numel();
  auto out = torch::empty({n}, keys.options().dtype(torch::kUInt8));
  launch_group_start((const uint64_t*)keys.data_ptr(), out.data_ptr<uint8_t>(), n,
                     cur_stream());
  return out;
}

static torch::Tensor pack_key_i64(torch::Tensor x) {
  CHECK_GPU(x);
  auto out = torch::empty_like(x);
  launch_pack_key_i64(x.data_ptr<int64_t>(), (uint64_t*)out.data_ptr(), x.numel(),
                      cur_stream());
  return out;
}

static torch::Tensor pack_key_2xi32(torch::Tensor hi, torch::Tensor lo) {
  CHECK_GPU_NONEMPTY(lo);
  CHECK_GPU(hi);
  auto out = torch::empty({hi.numel()}, hi.options().dtype(torch::kInt64));
  launch_pack_key_2xi32(hi.data_ptr<int32_t>(), lo.data_ptr<int32_t>(),
                        (uint64_t*)out.data_ptr(), hi.numel(), cur_stream());
  return out;
}

// ---- gathers ----------------------------------------------------------- //

// out[c][i] = cols[c][idx[i]] for every column, 16 columns per launch (the
// gather_fixed_multi binding). A column is 1-d of any 1/2/4/8-byte dtype,
// or [rows, es] whose es-wide rows move as one element.
static std::vector<torch::Tensor> gather_fixed(std::vector<torch::Tensor> cols,
                                               torch::Tensor idx) {
  CHECK_GPU(idx);
  int64_t n = idx.numel();
  std::vector<torch::Tensor> outs;
  size_t c = 0;
  while (c < cols.size()) {
    GatherTable tbl;
    tbl.ncols = 0;
    for (; c < cols.size() && tbl.ncols < 16; c++) {
      auto& col = cols[c];
      CHECK_GPU(col);
      bool wide = col.dim() == 2;
      int64_t es = col.element_size() * (wide ? col.size(1) : 1);
      TORCH_CHECK(es == 1 || es == 2 || es == 4 || es == 8,
                  "gather_fixed: unsupported elem size ", es);
      auto out = wide ? torch::empty({n, col.size(1)}, col.options())
                      : torch::empty({n}, col.options());
      tbl.src[tbl.ncols] = col.data_ptr();
      tbl.dst[tbl.ncols] = out.data_ptr();
      tbl.esize[tbl.ncols] = (int)es;
      tbl.ncols++;
      outs.push_back(out);
    }
    launch_gather_fixed_multi(tbl, idx.data_ptr<int64_t>(), n, cur_stream());
  }
  return outs;
}

// One column of gather_files: per file its buffer of rows[f] elements of
// `es` bytes, or nullptr for a file whose value is 1 in every row (a file
// without validity); dst holds idx.numel() elements.
struct FileColumn {
  std::vector<const void*> src;
  int es;
  void* dst;
};

// dst[c][i] = the row idx[i] of column c, where idx counts rows over the
// files in file order (rows[f] rows in file f): the gather of
// gather_fixed without a concatenated copy of the column. A launch takes 16
// columns and 16 files; with more files every 16 take a launch of their
// own, which writes the rows that fall into them. An idx outside all files
// leaves its output row unwritten.
static void gather_files_launch(const std::vector<FileColumn>& cols,
                                const std::vector<int64_t>& rows,
                                const torch::Tensor& idx) {
  const int64_t n = idx.numel();
  const size_t nfiles = rows.size();
  std::vector<int64_t> start(nfiles + 1, 0);
  for (size_t f = 0; f < nfiles; f++) start[f + 1] = start[f] + rows[f];
  for (size_t c0 = 0; c0 < cols.size(); c0 += GATHER_FILES_MAX_COLS) {
    for (size_t f0 = 0; f0 < nfiles; f0 += GATHER_FILES_MAX_FILES) {
      GatherFilesTable tbl = {};
      tbl.nfiles = (int)std::min<size_t>(GATHER_FILES_MAX_FILES, nfiles - f0);
      for (int f = 0; f <= tbl.nfiles; f++) tbl.start[f] = start[f0 + f];
      for (int f = tbl.nfiles; f < GATHER_FILES_MAX_FILES; f++) tbl.start[f + 1] = tbl.start[f];
      for (size_t c = c0; c < cols.size() && tbl.ncols < GATHER_FILES_MAX_COLS; c++) {
        const FileColumn& col = cols[c];
        TORCH_CHECK(col.es == 1 || col.es == 2 || col.es == 4 || col.es == 8,
                    "gather_files: unsupported elem size ", col.es);
        for (int f = 0; f < tbl.nfiles; f++) tbl.src[tbl.ncols][f] = col.src[f0 + f];
        tbl.dst[tbl.ncols] = col.dst;
        tbl.esize[tbl.ncols] = col.es;
        tbl.ncols++;
      }
      launch_gather_files(tbl, idx.data_ptr<int64_t>(), n, cur_stream());
    }
  }
}

// the gather_files binding: cols[c][f] is file f's part of column c (1-d,
// rows[f] elements of a 1/2/4/8-byte dtype) or None for a file of ones.
// Returns one tensor per column; with `outs` given, writes into those.
static std::vector<torch::Tensor> gather_files(
    std::vector<std::vector<c10::optional<torch::Tensor>>> cols,
    std::vector<int64_t> rows, torch::Tensor idx,
    c10::optional<std::vector<torch::Tensor>> outs) {
  CHECK_GPU(idx);
  TORCH_CHECK(idx.scalar_type() == torch::kInt64 && idx.dim() == 1,
              "gather_files: idx must be 1-d int64");
  TORCH_CHECK(!outs.has_value() || outs->size() == cols.size(),
              "gather_files: one output per column");
  const int64_t n = idx.numel();
  std::vector<FileColumn> fcs;
  std::vector<torch::Tensor> res;
  for (size_t c = 0; c < cols.size(); c++) {
    TORCH_CHECK(cols[c].size() == rows.size(), "gather_files: one part per file");
    FileColumn fc;
    torch::Tensor first;
    for (size_t f = 0; f < rows.size(); f++) {
      if (!cols[c][f].has_value()) {
        fc.src.push_back(nullptr);
        continue;
      }
      const torch::Tensor& t = *cols[c][f];
      CHECK_GPU(t);
      if (!first.defined()) first = t;
      TORCH_CHECK(t.dim() == 1 && t.numel() == rows[f] &&
                      t.scalar_type() == first.scalar_type(),
                  "gather_files: a part must be 1-d, of its file's row count "
                  "and of the column's dtype");
      fc.src.push_back(t.data_ptr());  // null for an empty part: no row reads it
    }
    TORCH_CHECK(first.defined(), "gather_files: a column of no parts");
    fc.es = (int)first.element_size();
    torch::Tensor out;
    if (outs.has_value()) {
      out = (*outs)[c];
      CHECK_GPU(out);
      TORCH_CHECK(out.dim() == 1 && out.numel() == n &&
                      out.scalar_type() == first.scalar_type(),
                  "gather_files: an output must be 1-d, of idx's size and of "
                  "the column's dtype");
    } else {
      out = torch::empty({n}, first.options());
    }
    fc.dst = out.data_ptr();
    fcs.push_back(std::move(fc));
    res.push_back(out);
  }
  gather_files_launch(fcs, rows, idx);
  return res;
}

// Rows idx of a string column -> (new_offsets, new_bytes). One host sync,
// at the byte total.
static std::pair<torch::Tensor, torch::Tensor> take_strings(
    torch::Tensor bytes, torch::Tensor offsets, torch::Tensor idx) {
  CHECK_GPU_NONEMPTY(bytes);
  CHECK_GPU(offsets);
  CHECK_GPU(idx);
  TORCH_CHECK(offsets.scalar_type() == torch::kInt64 && offsets.numel() >= 1 &&
                  idx.scalar_type() == torch::kInt64,
              "take_strings: offsets (rows + 1) and idx must be int64");
  int64_t n = idx.numel(), nrows = offsets.numel() - 1;
  auto lens = offsets.narrow(0, 1, nrows) - offsets.narrow(0, 0, nrows);
  auto new_offs = torch::zeros({n + 1}, offsets.options());
  new_offs.narrow(0, 1, n).copy_(at::cumsum(lens.index({idx}), 0));
  int64_t total = n ? new_offs[n].item<int64_t>() : 0;
  TORCH_CHECK(total == 0 || bytes.numel(), "take_strings: offsets past empty bytes");
  auto new_bytes = torch::empty({total}, offsets.options().dtype(torch::kUInt8));
  launch_gather_strings(opt_u8(bytes), offsets.data_ptr<int64_t>(),
                        idx.data_ptr<int64_t>(), new_offs.data_ptr<int64_t>(),
                        new_bytes.data_ptr<uint8_t>(), n, cur_stream());
  return {new_offs, new_bytes};
}

static torch::Tensor gather_strings(torch::Tensor src_bytes, torch::Tensor src_offsets,
                                    torch::Tensor idx, torch::Tensor dst_offsets) {
  CHECK_GPU_NONEMPTY(src_offsets);
  CHECK_GPU_NONEMPTY(idx);
  CHECK_GPU_NONEMPTY(dst_offsets);
  CHECK_GPU(src_bytes);
  int64_t n = idx.numel();
  int64_t total = dst_offsets.numel() ? dst_offsets[n].item<int64_t>() : 0;
  auto out = torch::empty({total}, src_bytes.options());
  launch_gather_strings(src_bytes.data_ptr<uint8_t>(), src_offsets.data_ptr<int64_t>(),
                        idx.data_ptr<int64_t>(), dst_offsets.data_ptr<int64_t>(),
                        out.data_ptr<uint8_t>(), n, cur_stream());
  return out;
}

static torch::Tensor bytes_ne_mask(torch::Tensor offsets, torch::Tensor bytes,
                                   torch::Tensor pattern) {
  CHECK_GPU_NONEMPTY(bytes);
  CHECK_GPU_NONEMPTY(pattern);
  CHECK_GPU(offsets);
  int64_t n = offsets.numel() - 1;
  auto out = torch::empty({n}, offsets.options().dtype(torch::kUInt8));
  launch_bytes_ne_mask(offsets.data_ptr<int64_t>(), bytes.data_ptr<uint8_t>(),
                       pattern.data_ptr<uint8_t>(), (int)pattern.numel(),
                       out.data_ptr<uint8_t>(), n, cur_stream());
  return out;
}

// ---- string predicates ------------------------------------------------ //

// One leaf predicate over a string column (str_pred.hip). The operand is
// what lakesoul_amd._cpp.str_pred_compile_* made, moved to the device.
// shape: "rows", "wave" or None (picked from the mean value length, which
// the tensor sizes give without a sync). No host sync, no status read-back.
// The thresholds are the measured crossovers of profiles/r07_gpu_str_pred.md:
// a compare that runs to a value's last byte is faster a wave per row from
// 1 KB values on, a LIKE that searches for a middle segment from 96 bytes on.
constexpr int64_t STR_PRED_WAVE_MEAN_LEN_CMP = 1024;
constexpr int64_t STR_PRED_WAVE_MEAN_LEN_LIKE = 96;

static bool str_pred_pick_wave(int64_t op, int64_t nrows, int64_t nbytes) {
  int64_t at = op >= lspred::OP_LIKE ? STR_PRED_WAVE_MEAN_LEN_LIKE
                                     : STR_PRED_WAVE_MEAN_LEN_CMP;
  return nrows > 0 && nbytes / nrows >= at;
}

static torch::Tensor str_pred_mask(torch::Tensor offsets, torch::Tensor bytes,
                                   c10::optional<torch::Tensor> validity,
                                   int64_t op, torch::Tensor op_bytes,
                                   torch::Tensor op_meta,
                                   c10::optional<std::string> shape,
                                   c10::optional<torch::Tensor> out) {
  CHECK_GPU(offsets);
  CHECK_GPU_NONEMPTY(bytes);
  CHECK_GPU_NONEMPTY(op_bytes);
  CHECK_GPU(op_meta);
  TORCH_CHECK(op >= 0 && op < lspred::OP_COUNT, "str_pred_mask: bad op");
  TORCH_CHECK(offsets.dim() == 1 && offsets.numel() >= 1, "str_pred_mask: offsets");
  TORCH_CHECK(bytes.scalar_type() == torch::kUInt8 &&
              op_bytes.scalar_type() == torch::kUInt8 &&
              op_meta.scalar_type() == torch::kInt32, "str_pred_mask: dtypes");
  TORCH_CHECK(op_meta.numel() >= lspred::min_meta((int)op),
              "str_pred_mask: short operand");
  int64_t n = offsets.numel() - 1;
  const uint8_t* vp = nullptr;
  if (validity && validity->numel()) {
    CHECK_GPU(*validity);
    TORCH_CHECK(validity->numel() == n &&
                (validity->scalar_type() == torch::kUInt8 ||
                 validity->scalar_type() == torch::kBool), "str_pred_mask: validity");
    vp = (const uint8_t*)validity->data_ptr();
  }
  torch::Tensor o;
  if (out) {
    o = *out;
    CHECK_GPU(o);
    TORCH_CHECK(o.scalar_type() == torch::kBool && o.numel() == n,
                "str_pred_mask: out must be n bools");
  } else {
    o = torch::empty({n}, offsets.options().dtype(torch::kBool));
  }
  int wave;
  if (shape) {
    TORCH_CHECK(*shape == "rows" || *shape == "wave", "str_pred_mask: shape");
    wave = *shape == "wave";
  } else {
    wave = str_pred_pick_wave(op, n, bytes.numel());
  }
  const uint8_t* bp = bytes.numel() ? bytes.data_ptr<uint8_t>() : nullptr;
  const uint8_t* obp = op_bytes.numel() ? op_bytes.data_ptr<uint8_t>() : nullptr;
  if (offsets.scalar_type() == torch::kInt32)
    launch_str_pred(offsets.data_ptr<int32_t>(), bp, bytes.numel(), vp, (int)op,
                    obp, op_bytes.numel(), op_meta.data_ptr<int32_t>(),
                    op_meta.numel(), wave, (uint8_t*)o.data_ptr(), n, cur_stream());
  else if (offsets.scalar_type() == torch::kInt64)
    launch_str_pred(offsets.data_ptr<int64_t>(), bp, bytes.numel(), vp, (int)op,
                    obp, op_bytes.numel(), op_meta.data_ptr<int32_t>(),
                    op_meta.numel(), wave, (uint8_t*)o.data_ptr(), n, cur_stream());
  else
    TORCH_CHECK(false, "str_pred_mask: offsets must be int32 or int64");
  return o;
}

// ---- segmented merge ops ---------------------------------------------- //

static std::vector<torch::Tensor> segmented_sum(torch::Tensor vals, torch::Tensor grp,
                                                torch::Tensor contrib, torch::Tensor validity,
                                                int64_t ngroups) {
  CHECK_GPU_NONEMPTY(grp);
  CHECK_GPU_NONEMPTY(contrib);
  CHECK_GPU_NONEMPTY(validity);
  CHECK_GPU(vals);
  int64_t n = vals.numel();
  auto sums = torch::zeros({ngroups}, vals.options());
  auto has_null = torch::zeros({ngroups}, vals.options().dtype(torch::kInt32));
  const uint8_t* cb = opt_u8(contrib);
  const uint8_t* vb = opt_u8(validity);
  switch (vals.scalar_type()) {
    case torch::kFloat:
      launch_segmented_sum<float, float>(vals.data_ptr<float>(), grp.data_ptr<int64_t>(), cb, vb, sums.data_ptr<float>(), has_null.data_ptr<int32_t>(), n, cur_stream());
      break;
    case torch::kDouble:
      launch_segmented_sum<double, double>(vals.data_ptr<double>(), grp.data_ptr<int64_t>(), cb, vb, sums.data_ptr<double>(), has_null.data_ptr<int32_t>(), n, cur_stream());
      break;
    case torch::kInt32:
      launch_segmented_sum<int32_t, int32_t>(vals.data_ptr<int32_t>(), grp.data_ptr<int64_t>(), cb, vb, sums.data_ptr<int32_t>(), has_null.data_ptr<int32_t>(), n, cur_stream());
      break;
    case torch::kInt64:
      launch_segmented_sum<int64_t, int64_t>(vals.data_ptr<int64_t>(), grp.data_ptr<int64_t>(), cb, vb, sums.data_ptr<int64_t>(), has_null.data_ptr<int32_t>(), n, cur_stream());
      break;
    default:
      TORCH_CHECK(false, "unsupported dtype for segmented_sum");
  }
  return {sums, has_null};
}

static torch::Tensor segmented_last(torch::Tensor grp, torch::Tensor contrib,
                                    torch::Tensor validity, int64_t ngroups, int64_t n) {
  CHECK_GPU_NONEMPTY(contrib);
  CHECK_GPU_NONEMPTY(validity);
  CHECK_GPU(grp);
  auto out = torch::zeros({ngroups}, grp.options());
  launch_segmented_last(grp.data_ptr<int64_t>(), opt_u8(contrib), opt_u8(validity),
                        out.data_ptr<int64_t>(), n, cur_stream());
  return out - 1;  // -1 = no contributing row
}

// ---- ANN scoring (MFMA) ------------------------------------------------ //

// X (n, K) bf16, Q (nq, K) bf16 -> f32 scores, (n, nq) or query-major
// (nq, n): the per-query top-k then reads contiguous rows (28 ms -> 2.5 ms
// for 5M x 64 k=10; benchmarks/topk_micro.py)
static torch::Tensor ann_scores(torch::Tensor X, torch::Tensor Q, bool query_major) {
  CHECK_GPU(X);
  CHECK_GPU(Q);
  TORCH_CHECK(X.scalar_type() == torch::kBFloat16 && Q.scalar_type() == torch::kBFloat16,
              "ann_scores expects bf16");
  int64_t n = X.size(0);
  int64_t nq = Q.size(0);
  int64_t K = X.size(1);
  TORCH_CHECK(Q.size(1) == K, "dim mismatch");
  TORCH_CHECK(K % 32 == 0, "K must be a multiple of 32");
  TORCH_CHECK(nq % 16 == 0, "nq must be a multiple of 16 (pad queries)");
  auto f32 = X.options().dtype(torch::kFloat32);
  auto out = query_major ? torch::empty({nq, n}, f32) : torch::empty({n, nq}, f32);
  (query_major ? launch_ann_scores_t : launch_ann_scores)(
      (const short*)X.data_ptr(), (const short*)Q.data_ptr(),
      out.data_ptr<float>(), n, (int32_t)nq, (int32_t)K, cur_stream());
  return out;
}

// jobs int64 [n,4] = {src_off, src_len, dst_off, dst_len}; returns
// (dst_buffer, status int32[n]) — status 0 = ok.
static std::vector<torch::Tensor> snappy_decompress(torch::Tensor src,
                                                    torch::Tensor jobs,
                                                    int64_t total_dst) {
  CHECK_GPU(src);
  CHECK_GPU(jobs);
  auto dst = torch::empty({total_dst}, src.options());
  auto status = torch::empty({jobs.size(0)}, src.options().dtype(torch::kInt32));
  launch_snappy_decompress(src.data_ptr<uint8_t>(), jobs.data_ptr<int64_t>(),
                           jobs.size(0), dst.data_ptr<uint8_t>(),
                           status.data_ptr<int32_t>(), cur_stream());
  return {dst, status};
}

// ---- string columns moved on the GPU (strings.hip) --------------------- //

// Read-backs of dictionary string byte totals by the unit decoder: one per
// unit that has such columns, however many (the sync-budget test reads it).
static std::atomic<int64_t> g_dict_total_readbacks{0};

// PLAIN stream `raw` + dense offsets (n + 1, device) -> `out` (total bytes)
static void strip_prefixes_into(const torch::Tensor& raw, const torch::Tensor& doff,
                                torch::Tensor& out) {
  int64_t n = doff.numel() - 1, total = out.numel();
  if (total == 0 || n <= 0) return;
  launch_strip_prefixes(raw.data_ptr<uint8_t>(), raw.numel(),
                        doff.data_ptr<int64_t>(), n, out.data_ptr<uint8_t>(),
                        total, cur_stream());
}

// direct binding: one host sync, at the byte total. `out`, when given, is
// where the bytes go (any alignment); it must hold exactly the total.
static torch::Tensor strip_prefixes(torch::Tensor raw, torch::Tensor doff,
                                    c10::optional<torch::Tensor> out) {
  CHECK_GPU_NONEMPTY(raw);
  CHECK_GPU_NONEMPTY(doff);
  TORCH_CHECK(raw.scalar_type() == torch::kUInt8 && raw.dim() == 1 &&
                  doff.scalar_type() == torch::kInt64 && doff.dim() == 1,
              "strip_prefixes: raw uint8 and dense offsets int64, 1-d");
  auto u8 = torch::TensorOptions().dtype(torch::kUInt8).device(
      doff.numel() ? doff.device() : raw.device());
  int64_t n = doff.numel() ? doff.numel() - 1 : 0;
  int64_t total = n > 0 ? doff[n].item<int64_t>() : 0;
  TORCH_CHECK(total >= 0 && total + 4 * n <= raw.numel(),
              "strip_prefixes: offsets past the raw stream");
  torch::Tensor o;
  if (out.has_value()) {
    o = *out;
    TORCH_CHECK(o.numel() == 0 || (o.is_cuda() && o.is_contiguous()),
                "strip_prefixes: out must be a contiguous GPU tensor");
    TORCH_CHECK(o.scalar_type() == torch::kUInt8 && o.numel() == total,
                "strip_prefixes: out must hold exactly ", total, " bytes");
  } else {
    o = torch::empty({total}, u8);
  }
  if (total) strip_prefixes_into(raw, doff, o);
  return o;
}

// A dictionary string column, first half: row offsets from the dense
// indices. status: int32 [1] device, or-ed into.
struct DictStr {
  torch::Tensor offsets, entry, dict_off, dict_bytes;
  int64_t nrows = 0;
};

static DictStr dict_str_offsets(const torch::Tensor& idx, const torch::Tensor& dict_off,
                                const torch::Tensor& dict_bytes,
                                const torch::Tensor& vmask, int64_t nrows,
                                torch::Tensor status) {
  DictStr ds;
  ds.nrows = nrows;
  ds.dict_off = dict_off;
  ds.dict_bytes = dict_bytes;
  auto i64 = dict_off.options().dtype(torch::kInt64);
  ds.offsets = torch::zeros({nrows + 1}, i64);
  ds.entry = torch::empty({nrows}, i64.dtype(torch::kInt32));
  if (nrows == 0) return ds;
  auto lens = torch::empty({nrows}, i64);
  torch::Tensor pos;
  if (vmask.defined()) pos = at::cumsum(vmask, 0, torch::kInt64) - 1;
  launch_dict_str_lens(idx.numel() ? idx.data_ptr<int32_t>() : nullptr, idx.numel(),
                       dict_off.data_ptr<int64_t>(), dict_off.numel() - 1,
                       vmask.defined() ? vmask.data_ptr<uint8_t>() : nullptr,
                       vmask.defined() ? pos.data_ptr<int64_t>() : nullptr, nrows,
                       lens.data_ptr<int64_t>(), ds.entry.data_ptr<int32_t>(),
                       status.data_ptr<int32_t>(), cur_stream());
  ds.offsets.narrow(0, 1, nrows).copy_(at::cumsum(lens, 0));
  return ds;
}

// second half, once the byte total is on the host
static torch::Tensor dict_str_bytes(const DictStr& ds, int64_t total) {
  auto out = torch::empty({total}, ds.dict_off.options().dtype(torch::kUInt8));
  if (total > 0)
    launch_dict_str_copy(opt_u8(ds.dict_bytes), ds.dict_bytes.numel(),
                         ds.dict_off.data_ptr<int64_t>(), ds.dict_off.numel() - 1,
                         ds.entry.data_ptr<int32_t>(),
                         ds.offsets.data_ptr<int64_t>(), ds.nrows,
                         out.data_ptr<uint8_t>(), total, cur_stream());
  return out;
}

// direct binding: dense idx (one per valid row) -> (row offsets, bytes,
// status int32 [1]); rows whose index is no entry are empty and set status
static std::vector<torch::Tensor> dict_strings(torch::Tensor idx, torch::Tensor dict_off,
                                               torch::Tensor dict_bytes,
                                               c10::optional<torch::Tensor> validity) {
  CHECK_GPU_NONEMPTY(idx);
  CHECK_GPU_NONEMPTY(dict_bytes);
  CHECK_GPU(dict_off);
  TORCH_CHECK(idx.scalar_type() == torch::kInt32 &&
                  dict_off.scalar_type() == torch::kInt64 && dict_off.numel() >= 1 &&
                  dict_bytes.scalar_type() == torch::kUInt8,
              "dict_strings: idx int32, dict_offsets int64 (entries + 1), dict_bytes uint8");
  torch::Tensor vmask;
  int64_t nrows = idx.numel();
  if (validity.has_value()) {
    nrows = validity->numel();
    if (nrows) {
      CHECK_GPU(*validity);
      TORCH_CHECK(validity->scalar_type() == torch::kUInt8, "dict_strings: validity uint8");
      vmask = *validity;
    }
  }
  auto status = torch::zeros({1}, dict_off.options().dtype(torch::kInt32));
  auto ds = dict_str_offsets(idx, dict_off, dict_bytes, vmask, nrows, status);
  int64_t total = nrows ? ds.offsets[nrows].item<int64_t>() : 0;
  return {ds.offsets, dict_str_bytes(ds, total), status};
}

// ---------------------------------------------------------------------- //
// Scan-unit decode: every (file, column) chunk of one unit into dense
// device columns. desc: int64 [nfiles*ncols, UD_NFIELDS] from
// _cpp.read_unit_raw (layout: unit_desc.h). The one chunk decoder under
// both read_unit_gpu paths: scan_unit_uselast below, and the python-driven
// merge through the decode_unit binding.
struct UnitCol {
  bool present = false, is_string = false, is_list = false;
  torch::Tensor data;             // fixed width: es bytes per row
  torch::Tensor offsets, bytes;   // string: byte offsets; list: ELEMENT offsets
  torch::Tensor validity;         // undefined = all valid
};

static std::vector<UnitCol> decode_unit_cols(
    const torch::Tensor& vals, const torch::Tensor& validity_buf,
    const torch::Tensor& dicts, const torch::Tensor& runs,
    const torch::Tensor& soffs, const torch::Tensor& desc, int64_t nfiles,
    int64_t ncols, const torch::Tensor& enc) {
  CHECK_GPU_NONEMPTY(validity_buf);
  CHECK_GPU_NONEMPTY(enc);
  CHECK_GPU_NONEMPTY(dicts);
  CHECK_GPU_NONEMPTY(runs);
  CHECK_GPU_NONEMPTY(soffs);
  CHECK_GPU(vals);
  TORCH_CHECK(desc.is_cpu() && desc.scalar_type() == torch::kInt64 &&
                  desc.dim() == 2 && desc.size(0) == nfiles * ncols &&
                  desc.size(1) == UD_NFIELDS,
              "decode_unit: desc must be a CPU int64 [nfiles*ncols, UD_NFIELDS] tensor");
  auto u8 = torch::TensorOptions().dtype(torch::kUInt8).device(vals.device());
  auto da = desc.accessor<int64_t, 2>();
  auto stream = cur_stream();
  torch::Tensor runs2 = runs.numel() ? runs.view({-1, 6}) : runs;
  TORCH_CHECK(enc.numel() == 0 ||
                  (enc.scalar_type() == torch::kInt64 && enc.numel() % 6 == 0),
              "decode_unit: enc must be an int64 [m, 6] tensor");
  const int64_t enc_rows = enc.numel() / 6;

  // dictionary string columns (UD_STR_DICT): their byte totals are known
  // only on the device. Every column's offsets are computed in the loop
  // below; the totals and statuses then come back in ONE copy for the whole
  // unit, and the bytes move after it.
  int64_t n_dict_str = 0;
  for (int64_t u = 0; u < nfiles * ncols; u++)
    if (da[u][UD_PRESENT] && da[u][UD_STR] == UD_STR_DICT) n_dict_str++;
  torch::Tensor dict_status;
  if (n_dict_str) dict_status = torch::zeros({n_dict_str}, u8.dtype(torch::kInt32));
  std::vector<std::pair<int64_t, DictStr>> dict_strs;

  std::vector<UnitCol> cols((size_t)(nfiles * ncols));
  for (int64_t u = 0; u < nfiles * ncols; u++) {
    UnitCol& out = cols[(size_t)u];
    const auto d = da[u];
    if (!d[UD_PRESENT]) continue;
    out.present = true;
    int64_t nv = d[UD_NUM_VALUES];
    bool has_null = d[UD_VALIDITY_OFF] >= 0 && d[UD_NULL_COUNT] > 0;
    if (has_null) out.validity = validity_buf.narrow(0, d[UD_VALIDITY_OFF], nv);
    const torch::Tensor& vmask = out.validity;
    if (d[UD_STR]) {
      // GPU string route: the host shipped prefixes / indices, the bytes
      // move here (strings.hip)
      TORCH_CHECK(d[UD_IS_STRING] && !d[UD_IS_LIST], "decode_unit: UD_STR on a non-string column");
      out.is_string = true;
      int64_t dn = d[UD_DENSE_N];
      TORCH_CHECK(dn >= 0 && dn <= nv && (has_null || dn == nv),
                  "decode_unit: bad dense count of a string column");
      TORCH_CHECK(d[UD_VAL_OFF] >= 0 && d[UD_VAL_LEN] >= 0 &&
                      d[UD_VAL_OFF] + d[UD_VAL_LEN] <= vals.numel(),
                  "decode_unit: string payload out of range");
      if (d[UD_STR] == UD_STR_PLAIN) {
        int64_t total = d[UD_SBYTES_LEN];
        TORCH_CHECK(d[UD_SOFF_OFF] >= 0 && d[UD_SOFF_OFF] + dn + 1 <= soffs.numel() &&
                        total >= 0 && total + 4 * dn == d[UD_VAL_LEN],
                    "decode_unit: string offsets out of range");
        auto doff = soffs.narrow(0, d[UD_SOFF_OFF], dn + 1);
        out.bytes = torch::empty({total}, u8);
        strip_prefixes_into(vals.narrow(0, d[UD_VAL_OFF], d[UD_VAL_LEN]), doff, out.bytes);
        if (has_null) {
          // row r starts where the dense value after its earlier valid rows does
          auto pos = at::clamp_max(
              at::cumsum(vmask, 0, torch::kInt64) - vmask.to(torch::kInt64), dn);
          out.offsets = at::cat({doff.index({pos}), doff.narrow(0, dn, 1)});
        } else {
          out.offsets = doff;
        }
      } else {
        TORCH_CHECK(d[UD_STR] == UD_STR_DICT, "decode_unit: unknown string tag ", d[UD_STR]);
        int64_t nent = d[UD_SBYTES_LEN];
        TORCH_CHECK(nent >= 0 && d[UD_SOFF_OFF] >= 0 &&
                        d[UD_SOFF_OFF] + nent + 1 <= soffs.numel() &&
                        d[UD_DICT_OFF] >= 0 && d[UD_DICT_LEN] >= 0 &&
                        d[UD_DICT_OFF] + d[UD_DICT_LEN] <= dicts.numel() &&
                        d[UD_RUN_OFF] >= 0 && d[UD_RUN_CNT] >= 0 &&
                        d[UD_RUN_OFF] + d[UD_RUN_CNT] <= runs.numel() / 6,
                    "decode_unit: string dictionary out of range");
        auto idx = torch::empty({dn}, u8.dtype(torch::kInt32));
        if (d[UD_RUN_CNT]) {
          auto rr = runs2.narrow(0, d[UD_RUN_OFF], d[UD_RUN_CNT]);
          launch_rle_expand(vals.data_ptr<uint8_t>(), rr.data_ptr<int64_t>(),
                            rr.size(0), idx.data_ptr<int32_t>(), dn, stream);
        }
        int64_t k = (int64_t)dict_strs.size();
        dict_strs.emplace_back(u, dict_str_offsets(
            idx, soffs.narrow(0, d[UD_SOFF_OFF], nent + 1),
            dicts.numel() ? dicts.narrow(0, d[UD_DICT_OFF], d[UD_DICT_LEN]) : dicts,
            vmask, nv, dict_status.narrow(0, k, 1)));
      }
      continue;
    }
    if (d[UD_IS_STRING] || d[UD_IS_LIST]) {
      out.is_string = d[UD_IS_STRING];
      out.is_list = d[UD_IS_LIST];
      out.offsets = soffs.narrow(0, d[UD_SOFF_OFF], nv + 1);
      out.bytes = vals.narrow(0, d[UD_SBYTES_OFF], d[UD_SBYTES_LEN]);
      continue;
    }
    int64_t es = d[UD_ESIZE];
    if (d[UD_ENC]) {
      // raw DELTA_BINARY_PACKED / BYTE_STREAM_SPLIT pages -> the DENSE
      // column (delta.hip); nulls then scatter like a PLAIN column
      int64_t np = d[UD_ENC_PAGES], nm = d[UD_ENC_CNT] - np, dn = d[UD_DENSE_N];
      TORCH_CHECK(es == 4 || es == 8, "decode_unit: encoded column of elem size ", es);
      TORCH_CHECK(np >= 0 && nm >= 0 && d[UD_ENC_OFF] >= 0 &&
                      d[UD_ENC_OFF] + d[UD_ENC_CNT] <= enc_rows,
                  "decode_unit: enc rows out of range (was the enc table passed?)");
      TORCH_CHECK(d[UD_VAL_OFF] >= 0 && d[UD_VAL_OFF] + d[UD_VAL_LEN] <= vals.numel(),
                  "decode_unit: encoded payload out of range");
      TORCH_CHECK(dn >= 0 && dn <= nv, "decode_unit: bad dense count");
      const int64_t* pages = enc.data_ptr<int64_t>() + d[UD_ENC_OFF] * 6;
      const int64_t* mbs = pages + np * 6;
      // payload reads are bounded by the END OF THIS COLUMN's region
      const int64_t vend = d[UD_VAL_OFF] + d[UD_VAL_LEN];
      auto dense = torch::empty({dn * es}, u8);
      if (d[UD_ENC] == 1) {
        TORCH_CHECK(nm == 0 || np > 0, "decode_unit: miniblocks without a page");
        torch::Tensor totals, csum;
        const int64_t *tp = nullptr, *cp = nullptr;
        if (nm) {
          totals = torch::empty({nm}, u8.dtype(torch::kInt64));
          if (es == 4)
            launch_delta_binary_pass1<uint32_t>(vals.data_ptr<uint8_t>(), vend, mbs, nm, (uint32_t*)dense.data_ptr(), dn, totals.data_ptr<int64_t>(), stream);
          else
            launch_delta_binary_pass1<uint64_t>(vals.data_ptr<uint8_t>(), vend, mbs, nm, (uint64_t*)dense.data_ptr(), dn, totals.data_ptr<int64_t>(), stream);
          csum = at::cumsum(totals, 0);
          tp = totals.data_ptr<int64_t>();
          cp = csum.data_ptr<int64_t>();
        }
        if (es == 4)
          launch_delta_binary_pass2<uint32_t>(pages, np, mbs, nm, tp, cp, (uint32_t*)dense.data_ptr(), dn, stream);
        else
          launch_delta_binary_pass2<uint64_t>(pages, np, mbs, nm, tp, cp, (uint64_t*)dense.data_ptr(), dn, stream);
      } else {
        TORCH_CHECK(d[UD_ENC] == 2 && nm == 0, "decode_unit: unknown encoding tag ", d[UD_ENC]);
        if (es == 4)
          launch_byte_stream_split<uint32_t>(vals.data_ptr<uint8_t>(), vend, pages, np, (uint32_t*)dense.data_ptr(), dn, stream);
        else
          launch_byte_stream_split<uint64_t>(vals.data_ptr<uint8_t>(), vend, pages, np, (uint64_t*)dense.data_ptr(), dn, stream);
      }
      if (has_null) {
        auto pos = at::cumsum(vmask, 0, torch::kInt64) - 1;
        out.data = torch::zeros({nv * es}, u8);
        scatter_valid_es(es, dense.data_ptr(), vmask.data_ptr<uint8_t>(),
                         pos.data_ptr<int64_t>(), out.data.data_ptr(), nv, stream);
      } else {
        TORCH_CHECK(dn == nv, "decode_unit: dense count differs from the row count");
        out.data = dense;
      }
    } else if (d[UD_IS_DICT]) {
      auto rr = runs2.narrow(0, d[UD_RUN_OFF], d[UD_RUN_CNT]);
      // run bit offsets are relative to the whole values buffer (they
      // already include this chunk's val_off, see read_unit.h)
      TORCH_CHECK(d[UD_VAL_OFF] + d[UD_VAL_LEN] <= vals.numel(),
                  "decode_unit: dict payload out of range");
      auto idx = torch::empty({d[UD_DENSE_N]}, u8.dtype(torch::kInt32));
      launch_rle_expand(vals.data_ptr<uint8_t>(), rr.data_ptr<int64_t>(),
                        rr.size(0), idx.data_ptr<int32_t>(), d[UD_DENSE_N], stream);
      auto dv = dicts.narrow(0, d[UD_DICT_OFF], d[UD_DICT_LEN]);
      out.data = torch::empty({nv * es}, u8);
      torch::Tensor pos;
      if (has_null) pos = at::cumsum(vmask, 0, torch::kInt64) - 1;
      dict_gather_scatter_es(es, dv.data_ptr(), idx.data_ptr<int32_t>(),
                             has_null ? vmask.data_ptr<uint8_t>() : nullptr,
                             has_null ? pos.data_ptr<int64_t>() : nullptr,
                             out.data.data_ptr(), nv, stream);
    } else {
      auto dense = vals.narrow(0, d[UD_VAL_OFF], d[UD_VAL_LEN]);
      if (has_null) {
        auto pos = at::cumsum(vmask, 0, torch::kInt64) - 1;
        out.data = torch::zeros({nv * es}, u8);
        scatter_valid_es(es, dense.data_ptr(), vmask.data_ptr<uint8_t>(),
                         pos.data_ptr<int64_t>(), out.data.data_ptr(), nv, stream);
      } else {
        out.data = dense;
      }
    }
  }
  if (!dict_strs.empty()) {
    std::vector<torch::Tensor> parts;
    for (auto& [u, ds] : dict_strs) parts.push_back(ds.offsets.narrow(0, ds.nrows, 1));
    parts.push_back(dict_status.to(torch::kInt64));
    auto host = at::cat(parts).cpu();  // the unit's one sync for these columns
    g_dict_total_readbacks++;
    const int64_t* h = host.data_ptr<int64_t>();
    const int64_t k = (int64_t)dict_strs.size();
    for (int64_t i = 0; i < k; i++)
      TORCH_CHECK(h[k + i] == 0,
                  "GPU dictionary string decode: index out of range (status ",
                  h[k + i], ", unit column ", dict_strs[(size_t)i].first, ")");
    for (int64_t i = 0; i < k; i++) {
      UnitCol& out = cols[(size_t)dict_strs[(size_t)i].first];
      out.offsets = dict_strs[(size_t)i].second.offsets;
      out.bytes = dict_str_bytes(dict_strs[(size_t)i].second, h[i]);
    }
  }
  return cols;
}

// the enc table is a trailing, optional argument of the unit bindings:
// units without GPU-decoded encodings never pass it
static torch::Tensor enc_or_empty(const c10::optional<torch::Tensor>& enc) {
  return enc.has_value() ? *enc : torch::empty({0}, torch::kInt64);
}

static py::object tensor_or_none(const torch::Tensor& t) {
  return t.defined() ? py::cast(t) : py::none();
}

// Unit columns as python entries; None for a column the file does not
// have. fixed width: (bytes_u8, validity_or_None); string and list:
// (offsets_i64, bytes_u8, validity_or_None) — list offsets count ELEMENTS.
static py::list unit_cols_to_py(const std::vector<UnitCol>& cols) {
  py::list out;
  for (auto& c : cols) {
    if (!c.present)
      out.append(py::none());
    else if (c.is_string || c.is_list)
      out.append(py::make_tuple(c.offsets, c.bytes, tensor_or_none(c.validity)));
    else
      out.append(py::make_tuple(c.data, tensor_or_none(c.validity)));
  }
  return out;
}

// One entry per unit column (row-major file, col).
static py::list decode_unit(torch::Tensor vals, torch::Tensor validity_buf,
                            torch::Tensor dicts, torch::Tensor runs,
                            torch::Tensor soffs, torch::Tensor desc,
                            int64_t nfiles, int64_t ncols,
                            c10::optional<torch::Tensor> enc) {
  std::vector<UnitCol> cols;
  {
    py::gil_scoped_release rel;
    cols = decode_unit_cols(vals, validity_buf, dicts, runs, soffs, desc,
                            nfiles, ncols, enc_or_empty(enc));
  }
  return unit_cols_to_py(cols);
}

// The string columns of a decoded unit (no absent or list columns)
// concatenated across their files in file order: offsets rebased onto the
// concatenated bytes. One UnitCol per column; a fixed-width column comes
// back empty (it is gathered straight from the per-file buffers, as every
// validity is: gather_files).
static std::vector<UnitCol> concat_unit_files(const std::vector<UnitCol>& flat,
                                              int64_t nfiles, int64_t ncols) {
  std::vector<UnitCol> out((size_t)ncols);
  for (int64_t c = 0; c < ncols; c++) {
    auto part = [&](int64_t f) -> const UnitCol& { return flat[(size_t)(f * ncols + c)]; };
    auto cat = [&](auto piece) {
      std::vector<torch::Tensor> parts;
      for (int64_t f = 0; f < nfiles; f++) parts.push_back(piece(f));
      return nfiles == 1 ? parts[0] : at::cat(parts, 0);
    };
    UnitCol& o = out[(size_t)c];
    o.present = true;
    o.is_string = part(0).is_string;
    if (!o.is_string) continue;
    int64_t byte_base = 0;
    o.offsets = cat([&](int64_t f) {
      auto offs = part(f).offsets;
      // later files: shift by the bytes before them, drop the leading 0
      if (f) offs = (offs + byte_base).narrow(0, 1, offs.numel() - 1);
      byte_base += part(f).bytes.numel();
      return offs;
    });
    o.bytes = cat([&](int64_t f) { return part(f).bytes; });
  }
  return out;
}

// C++ scan-unit driver (simple path): decode + UseLast merge + take for
// one unit entirely from C++ — the python per-unit op storm (GIL-bound)
// was the scan's critical path. Covers: integer single-PK (int64/int32),
// every-column UseLast, no CDC, no lists, no absent columns. Python falls
// back otherwise. One merged UnitCol per read column. Host syncs: one at
// the survivor count, one per string column at its byte total.
static std::vector<UnitCol> scan_unit_uselast_cols(
    const torch::Tensor& vals, const torch::Tensor& validity_buf,
    const torch::Tensor& dicts, const torch::Tensor& runs,
    const torch::Tensor& soffs, const torch::Tensor& desc, int64_t nfiles,
    int64_t ncols, int64_t pk_ci, int64_t pk_es, const torch::Tensor& enc) {
  TORCH_CHECK(nfiles >= 1 && pk_ci >= 0 && pk_ci < ncols && (pk_es == 4 || pk_es == 8),
              "scan_unit_uselast: bad pk column");
  auto flat = decode_unit_cols(vals, validity_buf, dicts, runs, soffs, desc,
                               nfiles, ncols, enc);
  for (auto& c : flat)
    TORCH_CHECK(c.present && !c.is_list,
                "scan_unit_uselast: absent or list column (fallback)");
  auto da = desc.accessor<int64_t, 2>();

  // merge the per-file keys as decoded; keep-last: source row of each
  // surviving key, as its index in the concatenation of the files
  std::vector<torch::Tensor> file_keys;
  std::vector<int64_t> rows;
  for (int64_t f = 0; f < nfiles; f++) {
    auto& pk = flat[(size_t)(f * ncols + pk_ci)].data;
    file_keys.push_back(pk.view(pk_es == 8 ? torch::kInt64 : torch::kInt32));
    rows.push_back(file_keys.back().numel());
  }
  auto src_idx = unit_merge_src_idx(std::move(file_keys));
  const int64_t n = src_idx.numel();

  // take the survivors: fixed-width data and the validity of every column
  // straight from the per-file buffers in one fused gather; only string
  // columns are concatenated first
  auto cols = concat_unit_files(flat, nfiles, ncols);
  auto u8 = torch::TensorOptions().dtype(torch::kUInt8).device(vals.device());
  std::vector<FileColumn> fcs;
  for (int64_t c = 0; c < ncols; c++) {
    auto part = [&](int64_t f) -> const UnitCol& { return flat[(size_t)(f * ncols + c)]; };
    UnitCol& o = cols[(size_t)c];
    if (!o.is_string) {
      int64_t es = da[c][UD_ESIZE];
      o.data = torch::empty({n * es}, u8);
      FileColumn fc;
      fc.es = (int)es;
      fc.dst = o.data.data_ptr();
      for (int64_t f = 0; f < nfiles; f++) {
        TORCH_CHECK(part(f).data.numel() == rows[(size_t)f] * es,
                    "scan_unit_uselast: a column's row count differs from the pk's");
        fc.src.push_back(part(f).data.data_ptr());
      }
      fcs.push_back(std::move(fc));
    }
    bool any_valid = false;
    for (int64_t f = 0; f < nfiles; f++) any_valid |= part(f).validity.defined();
    if (any_valid) {
      // files without a validity count as all ones
      o.validity = torch::empty({n}, u8);
      FileColumn fc;
      fc.es = 1;
      fc.dst = o.validity.data_ptr();
      for (int64_t f = 0; f < nfiles; f++) {
        auto& v = part(f).validity;
        TORCH_CHECK(!v.defined() || v.numel() == rows[(size_t)f],
                    "scan_unit_uselast: a validity's row count differs from the pk's");
        fc.src.push_back(v.defined() ? v.data_ptr() : nullptr);
      }
      fcs.push_back(std::move(fc));
    }
  }
  gather_files_launch(fcs, rows, src_idx);
  for (auto& c : cols)
    if (c.is_string)
      std::tie(c.offsets, c.bytes) = take_strings(c.bytes, c.offsets, src_idx);
  return cols;
}

// One entry per read column (the merged row count is implicit in the
// tensor sizes).
static py::list scan_unit_uselast(torch::Tensor vals, torch::Tensor validity_buf,
                                  torch::Tensor dicts, torch::Tensor runs,
                                  torch::Tensor soffs, torch::Tensor desc,
                                  int64_t nfiles, int64_t ncols, int64_t pk_ci,
                                  int64_t pk_es,
                                  c10::optional<torch::Tensor> enc) {
  std::vector<UnitCol> cols;
  {
    py::gil_scoped_release rel;  // long device-side section
    cols = scan_unit_uselast_cols(vals, validity_buf, dicts, runs, soffs, desc,
                                  nfiles, ncols, pk_ci, pk_es, enc_or_empty(enc));
  }
  return unit_cols_to_py(cols);
}

// decompress into an existing device buffer (jobs dst offsets index it)
static torch::Tensor snappy_decompress_into(torch::Tensor src, torch::Tensor jobs,
                                            torch::Tensor dst) {
  CHECK_GPU(src);
  CHECK_GPU(jobs);
  CHECK_GPU(dst);
  auto status = torch::empty({jobs.size(0)}, src.options().dtype(torch::kInt32));
  launch_snappy_decompress(src.data_ptr<uint8_t>(), jobs.data_ptr<int64_t>(),
                           jobs.size(0), dst.data_ptr<uint8_t>(),
                           status.data_ptr<int32_t>(), cur_stream());
  return status;
}

// GPU zstd: one wave per page, scratch literals buffer per block slot
static torch::Tensor zstd_decompress_into(torch::Tensor src, torch::Tensor jobs,
                                          torch::Tensor dst) {
  CHECK_GPU(src);
  CHECK_GPU(jobs);
  CHECK_GPU(dst);
  int64_t njobs = jobs.size(0);
  int64_t cap = 2048;
  if (const char* e = std::getenv("LAKESOUL_ZSTD_BLOCKS")) {
    int64_t v = atoll(e);
    if (v > 0) cap = v;
  }
  int64_t nblocks = njobs < cap ? njobs : cap;
  auto scratch = torch::empty({nblocks * lsz_gpu_litbuf_bytes()},
                              src.options().dtype(torch::kUInt8));
  auto status = torch::empty({njobs}, src.options().dtype(torch::kInt32));
  launch_zstd_decompress(src.data_ptr<uint8_t>(), jobs.data_ptr<int64_t>(),
                         njobs, dst.data_ptr<uint8_t>(),
                         scratch.data_ptr<uint8_t>(), nblocks,
                         status.data_ptr<int32_t>(), cur_stream());
  return status;
}

// the host-filled byte ranges [a, b) of a unit's values buffer, host to
// device on the current stream, in one GIL-free call: a unit whose pages
// decompress on the GPU leaves two such ranges per file, and as python
// slice copies they held the interpreter lock for 0.7 ms per unit
// (profiles/r03_gpu_huf.md). Tensor copies, so that the pinned buffer's
// allocator learns of the stream that still reads it.
static void copy_ranges_h2d(torch::Tensor host, torch::Tensor dev,
                            torch::Tensor ranges) {
  CHECK_GPU(dev);
  TORCH_CHECK(!host.is_cuda() && host.dim() == 1 && dev.dim() == 1 &&
                  host.scalar_type() == dev.scalar_type() &&
                  host.numel() == dev.numel(),
              "copy_ranges_h2d: two 1-d buffers of one size and type");
  TORCH_CHECK(!ranges.is_cuda() && ranges.scalar_type() == torch::kInt64 &&
                  ranges.dim() == 2 && ranges.size(1) == 2 &&
                  ranges.is_contiguous(),
              "copy_ranges_h2d: ranges is a host int64 [m][2]");
  const int64_t* r = ranges.data_ptr<int64_t>();
  const int64_t m = ranges.size(0), n = host.numel();
  for (int64_t i = 0; i < m; i++)
    TORCH_CHECK(0 <= r[2 * i] && r[2 * i] <= r[2 * i + 1] && r[2 * i + 1] <= n,
                "copy_ranges_h2d: range outside the buffer");
  py::gil_scoped_release rel;
  for (int64_t i = 0; i < m; i++) {
    int64_t a = r[2 * i], len = r[2 * i + 1] - a;
    if (len > 0) dev.narrow(0, a, len).copy_(host.narrow(0, a, len), true);
  }
}

// GPU decode of Huffman-only zstd pages (zstd_huf.hip): a workgroup per
// Huffman stream, straight into dst; no scratch. status[i] != 0: page i is
// not a valid Huffman-only page (part of its own range may be written).
static torch::Tensor zstd_huf_decompress_into(torch::Tensor src,
                                              torch::Tensor jobs,
                                              torch::Tensor dst) {
  CHECK_GPU(src);
  CHECK_GPU(jobs);
  CHECK_GPU(dst);
  TORCH_CHECK(jobs.dim() == 2 && jobs.size(1) == 4 && jobs.is_contiguous(),
              "jobs must be a contiguous [m][4] table");
  int64_t njobs = jobs.size(0);
  auto status = torch::empty({njobs}, src.options().dtype(torch::kInt32));
  launch_zstd_huf_decompress(src.data_ptr<uint8_t>(), jobs.data_ptr<int64_t>(),
                             njobs, dst.data_ptr<uint8_t>(),
                             status.data_ptr<int32_t>(), cur_stream());
  return status;
}

// GPU LZ4 (lz4.hip): LZ4_RAW page blocks, one wave per page, no scratch.
// jobs as for snappy. lz4_decompress_into writes into an existing device
// buffer; lz4_decompress allocates total_dst bytes and returns
// (dst, status) for direct tests. status[i] != 0: page i is not a valid
// block (part of its own output range may be written).
static torch::Tensor lz4_decompress_into(torch::Tensor src, torch::Tensor jobs,
                                         torch::Tensor dst) {
  CHECK_GPU(src);
  CHECK_GPU(jobs);
  CHECK_GPU(dst);
  TORCH_CHECK(jobs.dim() == 2 && jobs.size(1) == 4 && jobs.is_contiguous(),
              "jobs must be a contiguous [m][4] table");
  auto status = torch::empty({jobs.size(0)}, src.options().dtype(torch::kInt32));
  launch_lz4_decompress(src.data_ptr<uint8_t>(), jobs.data_ptr<int64_t>(),
                        jobs.size(0), dst.data_ptr<uint8_t>(),
                        status.data_ptr<int32_t>(), cur_stream());
  return status;
}

static std::vector<torch::Tensor> lz4_decompress(torch::Tensor src,
                                                 torch::Tensor jobs,
                                                 int64_t total_dst) {
  auto dst = torch::empty({total_dst}, src.options());
  return {dst, lz4_decompress_into(src, jobs, dst)};
}

// GPU GZIP (gzip.hip): GZIP pages (gzip members or a zlib stream), one wave
// per page, no scratch. jobs as for snappy. gzip_decompress_into writes
// into an existing device buffer; gzip_decompress allocates total_dst bytes
// and returns (dst, status) for direct tests. status[i] != 0: page i is not
// a valid page (part of its own output range may be written). CRC32 and
// Adler-32 are not checked on this route.
static torch::Tensor gzip_decompress_into(torch::Tensor src, torch::Tensor jobs,
                                          torch::Tensor dst) {
  CHECK_GPU(src);
  CHECK_GPU(jobs);
  CHECK_GPU(dst);
  TORCH_CHECK(jobs.dim() == 2 && jobs.size(1) == 4 && jobs.is_contiguous(),
              "jobs must be a contiguous [m][4] table");
  auto status = torch::empty({jobs.size(0)}, src.options().dtype(torch::kInt32));
  launch_gzip_decompress(src.data_ptr<uint8_t>(), jobs.data_ptr<int64_t>(),
                         jobs.size(0), dst.data_ptr<uint8_t>(),
                         status.data_ptr<int32_t>(), cur_stream());
  return status;
}

static std::vector<torch::Tensor> gzip_decompress(torch::Tensor src,
                                                  torch::Tensor jobs,
                                                  int64_t total_dst) {
  auto dst = torch::empty({total_dst}, src.options());
  return {dst, gzip_decompress_into(src, jobs, dst)};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("ann_scores", [](torch::Tensor X, torch::Tensor Q) { return ann_scores(X, Q, false); });
  m.def("ann_scores_t", [](torch::Tensor X, torch::Tensor Q) { return ann_scores(X, Q, true); });
  m.def("zstd_decompress_into", &zstd_decompress_into);
  m.def("zstd_huf_decompress_into", &zstd_huf_decompress_into);
  m.def("copy_ranges_h2d", &copy_ranges_h2d);
  m.def("str_chunk_keys", [](torch::Tensor offsets, torch::Tensor bytes,
                             int64_t chunk) {
    CHECK_GPU(offsets);
    CHECK_GPU(bytes);
    int64_t n = offsets.numel() - 1;
    auto out = torch::empty({n}, offsets.options().dtype(torch::kInt64));
    launch_str_chunk_keys(offsets.data_ptr<int64_t>(),
                          bytes.data_ptr<uint8_t>(), chunk,
                          out.data_ptr<int64_t>(), n, cur_stream());
    return out;
  });
  m.def("hamming_scores", [](torch::Tensor codes, torch::Tensor qcodes) {
    CHECK_GPU(codes);
    CHECK_GPU(qcodes);
    int64_t n = codes.size(0);
    int nq = (int)qcodes.size(0);
    int words = (int)codes.size(1);
    TORCH_CHECK(words <= 16 && qcodes.size(1) == words);
    auto out = torch::empty({n, nq}, codes.options().dtype(torch::kInt32));
    launch_hamming_scores((const uint64_t*)codes.data_ptr<int64_t>(),
                          (const uint64_t*)qcodes.data_ptr<int64_t>(),
                          out.data_ptr<int32_t>(), n, nq, words, cur_stream());
    return out;
  });
  m.def("fastscan_est", [](torch::Tensor bits, torch::Tensor q, int64_t dim,
                           torch::Tensor f_add, torch::Tensor f_rescale,
                           torch::Tensor cl_of_row, torch::Tensor g_add,
                           torch::Tensor c1_sum_q) {
    // fused RaBitQ stage-1: (nq, n) estimated distances in one pass
    CHECK_GPU(bits);
    CHECK_GPU(q);
    CHECK_GPU(f_add);
    CHECK_GPU(f_rescale);
    CHECK_GPU(cl_of_row);
    CHECK_GPU(g_add);
    CHECK_GPU(c1_sum_q);
    TORCH_CHECK(bits.dtype() == torch::kUInt8 && bits.is_contiguous());
    TORCH_CHECK(cl_of_row.dtype() == torch::kInt32);
    int64_t m = bits.size(0);
    int w = (int)bits.size(1);
    int nq = (int)q.size(0);
    int g = (int)((dim + 3) / 4);
    int kc = (int)g_add.size(1);
    TORCH_CHECK(w == (dim + 7) / 8, "bits width mismatch");
    TORCH_CHECK(g_add.size(0) == nq && c1_sum_q.size(0) == nq);
    TORCH_CHECK(f_add.size(0) == m && f_rescale.size(0) == m &&
                cl_of_row.size(0) == m);
    auto qp = torch::zeros({nq, (int64_t)g * 4}, q.options());
    qp.slice(1, 0, dim).copy_(q);
    auto qg = qp.view({nq, g, 4});
    static float pat_host[16 * 4];
    static bool pat_init = false;
    if (!pat_init) {
      for (int v = 0; v < 16; v++)
        for (int j = 0; j < 4; j++) pat_host[v * 4 + j] = (float)((v >> j) & 1);
      pat_init = true;
    }
    auto pat = torch::from_blob(pat_host, {16, 4},
                                torch::TensorOptions().dtype(torch::kFloat32))
                   .to(q.device());
    auto lut = torch::matmul(qg, pat.t()).contiguous();
    auto out = torch::empty({nq, m}, q.options());
    launch_fastscan_est(
        bits.data_ptr<uint8_t>(), lut.data_ptr<float>(),
        f_add.contiguous().data_ptr<float>(),
        f_rescale.contiguous().data_ptr<float>(),
        cl_of_row.contiguous().data_ptr<int32_t>(),
        g_add.contiguous().data_ptr<float>(),
        c1_sum_q.contiguous().data_ptr<float>(), out.data_ptr<float>(), m, nq,
        w, g, kc, cur_stream());
    return out;
  });
  m.def("fastscan_ex_dot_pairs",
        [](torch::Tensor ex, torch::Tensor cand, torch::Tensor q,
           int64_t dim) {
    // ex (n, wn) uint8 (FULL table); cand (nq, C) int64 row indices
    // (-1 = missing); q (nq, dim) f32 -> (nq, C) f32 per-pair dots
    CHECK_GPU(ex);
    CHECK_GPU(cand);
    CHECK_GPU(q);
    TORCH_CHECK(ex.dtype() == torch::kUInt8 && ex.is_contiguous());
    TORCH_CHECK(cand.dtype() == torch::kInt64);
    TORCH_CHECK(q.dtype() == torch::kFloat32);
    int wn = (int)ex.size(1);
    int nq = (int)cand.size(0);
    int C = (int)cand.size(1);
    TORCH_CHECK(wn == (dim + 1) / 2, "ex width mismatch");
    TORCH_CHECK(q.size(0) == nq, "query count mismatch");
    auto qc = q.contiguous();
    auto cc = cand.contiguous();
    auto out = torch::empty({nq, C}, q.options());
    launch_fastscan_ex_dot_pairs(ex.data_ptr<uint8_t>(),
                                 cc.data_ptr<int64_t>(),
                                 qc.data_ptr<float>(), out.data_ptr<float>(),
                                 C, nq, wn, (int)dim, cur_stream());
    return out;
  });
  m.def("strip_prefixes", &strip_prefixes, py::arg("raw"), py::arg("dense_offsets"),
        py::arg("out") = py::none());
  m.def("dict_strings", &dict_strings, py::arg("idx"), py::arg("dict_offsets"),
        py::arg("dict_bytes"), py::arg("validity") = py::none());
  m.def("dict_total_readbacks", []() { return g_dict_total_readbacks.load(); },
        "read-backs of dictionary string byte totals by the unit decoder so far");
  m.def("snappy_decompress", &snappy_decompress);
  m.def("snappy_decompress_into", &snappy_decompress_into);
  m.def("lz4_decompress", &lz4_decompress);
  m.def("lz4_decompress_into", &lz4_decompress_into);
  m.def("gzip_decompress", &gzip_decompress);
  m.def("gzip_decompress_into", &gzip_decompress_into);
  m.def("scan_unit_uselast", &scan_unit_uselast, py::arg("vals"),
        py::arg("validity"), py::arg("dicts"), py::arg("runs"), py::arg("soffs"),
        py::arg("desc"), py::arg("nfiles"), py::arg("ncols"), py::arg("pk_ci"),
        py::arg("pk_es"), py::arg("enc") = py::none());
  m.def("decode_unit", &decode_unit, py::arg("vals"), py::arg("validity"),
        py::arg("dicts"), py::arg("runs"), py::arg("soffs"), py::arg("desc"),
        py::arg("nfiles"), py::arg("ncols"), py::arg("enc") = py::none());
  m.doc() = "lakesoul_amd gfx950 HIP kernels";
  m.def("hash_fixed_column", &hash_fixed_column);
  m.def("hash_string_column", &hash_string_column);
  m.def("bucket_ids", &bucket_ids);
  m.def("merge_sorted_keys", &merge_key_streams);
  m.def("unit_merge_src_idx", &unit_merge_src_idx, py::arg("keys"));
  m.def("gather_files", &gather_files, py::arg("cols"), py::arg("rows"),
        py::arg("idx"), py::arg("outs") = py::none());
  m.def("group_start_mask", &group_start_mask);
  m.def("pack_key_i64", &pack_key_i64);
  m.def("pack_key_2xi32", &pack_key_2xi32);
  m.def("gather_fixed_multi", &gather_fixed);
  m.def("take_strings", &take_strings);
  m.def("gather_strings", &gather_strings);
  m.def("bytes_ne_mask", &bytes_ne_mask);
  m.def("str_pred_mask", &str_pred_mask, py::arg("offsets"), py::arg("bytes"),
        py::arg("validity"), py::arg("op"), py::arg("op_bytes"),
        py::arg("op_meta"), py::arg("shape") = py::none(),
        py::arg("out") = py::none());
  m.def("str_pred_lds_budget", []() { return str_pred_lds_budget(); });
  m.def("str_pred_pick_shape", [](int64_t op, int64_t nrows, int64_t nbytes) {
    return std::string(str_pred_pick_wave(op, nrows, nbytes) ? "wave" : "rows");
  }, py::arg("op"), py::arg("nrows"), py::arg("nbytes"),
        "the shape str_pred_mask takes when none is forced");
  m.def("segmented_sum", &segmented_sum);
  m.def("segmented_last", &segmented_last);
}
