// Host-side interface of the gfx950 kernels: every launcher the torch
// bindings (hip_module.cc) call, declared once and included by the .hip
// file that defines it: a definition that drifts from its declaration
// leaves an undefined symbol, and the extension fails to import.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lakesoul {

// kernels.hip — hashing
void launch_hash_fixed(int dt, const void* data, const uint8_t* validity,
                       const int64_t* prev, int64_t* out, int64_t n, int first,
                       hipStream_t s);
void launch_hash_string(const int32_t* offsets, const uint8_t* bytes,
                        const uint8_t* validity, const int64_t* prev,
                        int64_t* out, int64_t n, int first, hipStream_t s);
void launch_bucket_ids(const int64_t* hashes, int32_t* out, int64_t n,
                       uint32_t nb, hipStream_t s);

// kernels.hip — decode
void launch_rle_expand(const uint8_t* payload, const int64_t* runs,
                       int64_t nruns, int32_t* out, int64_t n, hipStream_t s);
template <typename T>
void launch_dict_gather_scatter(const T* dict, const int32_t* idx,
                                const uint8_t* validity, const int64_t* pos,
                                T* out, int64_t n, hipStream_t s);
template <typename T>
void launch_scatter_valid(const T* dense, const uint8_t* validity,
                          const int64_t* pos, T* out, int64_t n, hipStream_t s);

// kernels.hip — merge. One launch merges up to MERGE_PAIRS_PER_LAUNCH pairs
// of sorted (key, row) streams, a 2048-row tile per workgroup (the plan:
// ../cpp/merge_plan.h). MergeTable is passed BY VALUE into
// merge_round_kernel: this is its only definition.
constexpr int MERGE_PAIRS_PER_LAUNCH = 16;
struct MergePairArg {
  // a stream with rows == nullptr is an input stream: its keys are in the
  // launch's key format and the row value of element i is base + i. Any
  // other stream holds packed u64 keys and stored row values. A is the
  // older stream: first on equal keys.
  const void* kA;
  const int64_t* rA;
  int64_t nA, baseA;
  const void* kB;
  const int64_t* rB;
  int64_t nB, baseB;
  uint64_t* kOut;  // nA + nB packed keys; unused by the keep-last round
  int64_t* rOut;   // nA + nB row values (keep-last round: tile slots)
  int64_t first_tile;  // tiles of this launch before this pair
};
struct MergeTable {
  MergePairArg p[MERGE_PAIRS_PER_LAUNCH];
  int npairs;
  int64_t ntiles;        // tiles of all pairs of this launch
  int64_t* tile_counts;  // keep-last round only: survivors per tile
};
enum MergeKeyFormat { MERGE_KEY_I64 = 0, MERGE_KEY_I32 = 1, MERGE_KEY_PACKED = 2 };
// key_format: how input streams store keys. int64/int32 keys are made
// order-preserving unsigned in registers (sign bit flipped, int32 widened).
void launch_merge_round(const MergeTable& tbl, int key_format, hipStream_t s);
// The last round of a UseLast merge: table of ONE pair (B may be empty).
// Writes no keys: of every run of equal keys only the last row survives;
// tile t's surviving row values go to rOut[t * 2048 ...), their number to
// tile_counts[t].
void launch_merge_round_keep_last(const MergeTable& tbl, int key_format,
                                  hipStream_t s);
// out[csum[t] - counts[t] + i] = slots[t * 2048 + i] for i < counts[t]
// (csum: inclusive prefix sum of counts)
void launch_compact_tiles(const int64_t* slots, const int64_t* counts,
                          const int64_t* csum, int64_t ntiles, int64_t* out,
                          hipStream_t s);
void launch_group_start(const uint64_t* keys, uint8_t* start, int64_t n, hipStream_t s);
void launch_pack_key_i64(const int64_t* x, uint64_t* out, int64_t n, hipStream_t s);
void launch_pack_key_2xi32(const int32_t* hi, const int32_t* lo, uint64_t* out,
                           int64_t n, hipStream_t s);

// kernels.hip — gathers. GatherTable is passed BY VALUE into
// gather_fixed_multi_kernel: this is its only definition.
struct GatherTable {
  const void* src[16];
  void* dst[16];
  int esize[16];
  int ncols;
};
void launch_gather_fixed_multi(const GatherTable& tbl, const int64_t* idx,
                               int64_t n, hipStream_t s);
// gather from per-file buffers: idx[i] is a row of the concatenation of the
// files in file order; file f holds rows [start[f], start[f + 1]). Rows
// outside [start[0], start[nfiles]) are left to another launch. A null
// source pointer stands for a file of ones (a file without validity).
// Passed BY VALUE into gather_files_kernel: this is its only definition.
constexpr int GATHER_FILES_MAX_COLS = 16;
constexpr int GATHER_FILES_MAX_FILES = 16;
struct GatherFilesTable {
  const void* src[GATHER_FILES_MAX_COLS][GATHER_FILES_MAX_FILES];
  void* dst[GATHER_FILES_MAX_COLS];
  int esize[GATHER_FILES_MAX_COLS];
  int64_t start[GATHER_FILES_MAX_FILES + 1];
  int ncols, nfiles;
};
void launch_gather_files(const GatherFilesTable& tbl, const int64_t* idx,
                         int64_t n, hipStream_t s);
void launch_gather_strings(const uint8_t* src_bytes, const int64_t* src_off,
                           const int64_t* idx, const int64_t* dst_off,
                           uint8_t* dst_bytes, int64_t n, hipStream_t s);
void launch_bytes_ne_mask(const int64_t* offsets, const uint8_t* bytes,
                          const uint8_t* pattern, int plen, uint8_t* out,
                          int64_t n, hipStream_t s);

// kernels.hip — segmented merge operators
template <typename T, typename ACC>
void launch_segmented_sum(const T* vals, const int64_t* grp, const uint8_t* contrib,
                          const uint8_t* validity, ACC* out_sum,
                          int32_t* out_has_null, int64_t n, hipStream_t s);
void launch_segmented_last(const int64_t* grp, const uint8_t* contrib,
                           const uint8_t* validity, int64_t* out_idx, int64_t n,
                           hipStream_t s);

// kernels.hip — string-PK sort keys, binary-code scorer
void launch_str_chunk_keys(const int64_t* offsets, const uint8_t* bytes,
                           int64_t chunk, int64_t* out, int64_t n,
                           hipStream_t s);
void launch_hamming_scores(const uint64_t* codes, const uint64_t* qcodes,
                           int32_t* out, int64_t n, int nq, int words,
                           hipStream_t s);

// ann.hip
void launch_ann_scores(const short* X, const short* Q, float* out, int64_t n,
                       int32_t nq, int32_t K, hipStream_t s);
void launch_ann_scores_t(const short* X, const short* Q, float* out, int64_t n,
                         int32_t nq, int32_t K, hipStream_t s);

// fastscan.hip
void launch_fastscan_est(const uint8_t* bits, const float* lut,
                         const float* f_add, const float* f_rescale,
                         const int32_t* cl_of_row, const float* g_add,
                         const float* c1_sum_q, float* out, int64_t m,
                         int32_t nq, int32_t w, int32_t g,
                         int32_t n_clusters, hipStream_t s);
void launch_fastscan_ex_dot_pairs(const uint8_t* ex, const int64_t* cand,
                                  const float* qv, float* out, int32_t C,
                                  int32_t nq, int32_t wn, int32_t dim,
                                  hipStream_t s);

// delta.hip — raw DELTA_BINARY_PACKED / BYTE_STREAM_SPLIT pages; table
// rows int64 [.][6] as laid out in ../cpp/read_unit.h (`enc`); T is
// uint32_t or uint64_t; `out` holds dense_n values
template <typename T>
void launch_delta_binary_pass1(const uint8_t* payload, int64_t vals_len,
                               const int64_t* mbs, int64_t nmb, T* out,
                               int64_t dense_n, int64_t* totals, hipStream_t s);
template <typename T>
void launch_delta_binary_pass2(const int64_t* pages, int64_t npages,
                               const int64_t* mbs, int64_t nmb,
                               const int64_t* totals, const int64_t* csum, T* out,
                               int64_t dense_n, hipStream_t s);
template <typename T>
void launch_byte_stream_split(const uint8_t* payload, int64_t vals_len,
                              const int64_t* pages, int64_t npages, T* out,
                              int64_t dense_n, hipStream_t s);

// strings.hip — byte-parallel segment copy of string columns (the GPU
// string route of ../cpp/read_unit.h). Offsets tables hold one more entry
// than values / rows / entries and start at 0; `dst` holds `total` bytes.
// Every source read is checked against raw_len / dict_len.
void launch_strip_prefixes(const uint8_t* raw, int64_t raw_len,
                           const int64_t* dense_off, int64_t n, uint8_t* dst,
                           int64_t total, hipStream_t s);
// per row: value length and dictionary entry (-1: null row or bad index);
// pos[r] = dense index of valid row r (read only with a validity);
// *status gets bit 0 for an index that is no entry, bit 1 for a valid row
// with no stored index
void launch_dict_str_lens(const int32_t* idx, int64_t n_idx,
                          const int64_t* dict_off, int64_t nent,
                          const uint8_t* validity, const int64_t* pos,
                          int64_t nrows, int64_t* lens, int32_t* entry,
                          int32_t* status, hipStream_t s);
void launch_dict_str_copy(const uint8_t* dict_bytes, int64_t dict_len,
                          const int64_t* dict_off, int64_t nent,
                          const int32_t* entry, const int64_t* row_off,
                          int64_t nrows, uint8_t* dst, int64_t total,
                          hipStream_t s);

// str_pred.hip — one leaf string predicate (../cpp/str_pred.h: ops and the
// compiled operand op_bytes / op_meta) over an offsets + bytes column;
// OffT is int32_t or int64_t and offsets[0] need not be 0; out[i] =
// validity[i] && pred(row i). wave_shape: a wave per row instead of a
// thread per row. An operand of at most STR_PRED_LDS_BUDGET bytes is staged
// in LDS.
constexpr int64_t STR_PRED_LDS_BUDGET = 16384;
int64_t str_pred_lds_budget();
template <typename OffT>
void launch_str_pred(const OffT* offsets, const uint8_t* bytes, int64_t nbytes,
                     const uint8_t* validity, int op, const uint8_t* op_bytes,
                     int64_t op_nbytes, const int32_t* op_meta,
                     int64_t op_nmeta, int wave_shape, uint8_t* out, int64_t n,
                     hipStream_t s);

// snappy.hip, lz4.hip, gzip.hip, zstd.hip, zstd_huf.hip
void launch_snappy_decompress(const uint8_t* src, const int64_t* jobs,
                              int64_t njobs, uint8_t* dst, int32_t* status,
                              hipStream_t s);
// LZ4_RAW page blocks; jobs as for snappy. A page that is not a valid
// block gets a non-zero status (it may be partly written, inside its own
// output range)
void launch_lz4_decompress(const uint8_t* src, const int64_t* jobs,
                           int64_t njobs, uint8_t* dst, int32_t* status,
                           hipStream_t s);
// GZIP pages (gzip members or a zlib stream); jobs as for snappy. Framing,
// ISIZE and the output length are checked, CRC32 and Adler-32 are not. A
// page that fails gets a non-zero status (it may be partly written, inside
// its own output range)
void launch_gzip_decompress(const uint8_t* src, const int64_t* jobs,
                            int64_t njobs, uint8_t* dst, int32_t* status,
                            hipStream_t s);
void launch_zstd_decompress(const uint8_t* src, const int64_t* jobs,
                            int64_t njobs, uint8_t* dst, uint8_t* scratch,
                            int64_t nblocks, int32_t* status, hipStream_t s);
int64_t lsz_gpu_litbuf_bytes();
// Huffman-only zstd pages (lszstd::huf_only_frame); any other page gets
// status 1 (a page whose streams are not all valid may be partly written,
// inside its own output range)
void launch_zstd_huf_decompress(const uint8_t* src, const int64_t* jobs,
                                int64_t njobs, uint8_t* dst, int32_t* status,
                                hipStream_t s);

}  // namespace lakesoul
