// MI355X (gfx950/CDNA4) kernels for the lakehouse engine — written
// directly in HIP for 64-wide wavefronts; no CUDA-compat paths.
//
// Kernel inventory (SURVEY.md §2.3 mapping):
//  - spark murmur3-32 hashing (bucket scatter)       <- utils/hash/
//  - RLE/bit-packed + dictionary decode              <- parquet decode path
//  - validity scatter (nullable column materialize)
//  - pairwise merge-path sorted merge + dedup        <- MOR SortedStreamMerger
//  - segmented merge operators (UseLast via dedup; sum ops)
//  - multi-column gather (payload materialization after key merge)
//  - string gather / CDC filter
//
// Design notes (per /opt/skills/guides/cdna_hip_programming.md):
//  - memory-bound kernels: grid-stride, <=2048 workgroups, vectorized
//    where layout permits (G11/G13);
//  - merge-path kernel stages key and row tiles in LDS (G3), 2048-element
//    tiles, 256 threads x 8 elements/thread, one launch per merge round;
//  - all block sizes are multiples of 64 (wave64).

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../cpp/merge_plan.h"
#include "../cpp/murmur3.h"
#include "kernels.h"

namespace lakesoul {

#define LS_THREADS 256
#define LS_MAX_BLOCKS 2048

static inline int ls_blocks(int64_t n, int per_thread = 1) {
  int64_t b = (n + (int64_t)LS_THREADS * per_thread - 1) / ((int64_t)LS_THREADS * per_thread);
  if (b > LS_MAX_BLOCKS) b = LS_MAX_BLOCKS;
  if (b < 1) b = 1;
  return (int)b;
}

// ===================================================================== //
// murmur3 hashing
// ===================================================================== //

// dtype codes: 0=u8/bool, 1=i8, 2=i16, 3=i32, 4=i64, 5=f32, 6=f64
template <int DT>
__global__ void hash_fixed_kernel(const void* __restrict__ data,
                                  const uint8_t* __restrict__ validity,
                                  const int64_t* __restrict__ prev,
                                  int64_t* __restrict__ out, int64_t n,
                                  int first) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t seed = first ? kHashSeed : (uint32_t)prev[i];
    if (validity && !validity[i]) {
      out[i] = first ? 0 : (int64_t)seed;
      continue;
    }
    uint32_t h;
    if constexpr (DT == 0) h = spark_hash_u32(((const uint8_t*)data)[i], seed);
    else if constexpr (DT == 1) h = spark_hash_u32((uint32_t)(int32_t)((const int8_t*)data)[i], seed);
    else if constexpr (DT == 2) h = spark_hash_u32((uint32_t)(int32_t)((const int16_t*)data)[i], seed);
    else if constexpr (DT == 3) h = spark_hash_u32((uint32_t)((const int32_t*)data)[i], seed);
    else if constexpr (DT == 4) h = spark_hash_u64((uint64_t)((const int64_t*)data)[i], seed);
    else if constexpr (DT == 5) h = spark_hash_f32(((const float*)data)[i], seed);
    else h = spark_hash_f64(((const double*)data)[i], seed);
    out[i] = (int64_t)h;
  }
}

__global__ void hash_string_kernel(const int32_t* __restrict__ offsets,
                                   const uint8_t* __restrict__ bytes,
                                   const uint8_t* __restrict__ validity,
                                   const int64_t* __restrict__ prev,
                                   int64_t* __restrict__ out, int64_t n,
                                   int first) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t seed = first ? kHashSeed : (uint32_t)prev[i];
    if (validity && !validity[i]) {
      out[i] = first ? 0 : (int64_t)seed;
      continue;
    }
    out[i] = (int64_t)spark_hash_bytes(bytes + offsets[i],
                                       offsets[i + 1] - offsets[i], seed);
  }
}

__global__ void bucket_ids_kernel(const int64_t* __restrict__ hashes,
                                  int32_t* __restrict__ out, int64_t n,
                                  uint32_t nbuckets) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    out[i] = (int32_t)((uint32_t)hashes[i] % nbuckets);
  }
}

// ===================================================================== //
// RLE / bit-packed hybrid expansion (dictionary indices, levels)
// ===================================================================== //

// runs: int64 [nruns][6] =
//   {out_off, n, is_literal, value_or_bitoff, bit_width, dict_elem_bias}
// repeat-run values arrive pre-biased; literal unpacks get bias added here.
// payload must be padded by >=8 bytes past the last literal bit.
__global__ void rle_expand_kernel(const uint8_t* __restrict__ payload,
                                  const int64_t* __restrict__ runs,
                                  int64_t nruns, int32_t* __restrict__ out,
                                  int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    // binary search run containing output index i
    int64_t lo = 0, hi = nruns - 1;
    while (lo < hi) {
      int64_t mid = (lo + hi + 1) >> 1;
      if (runs[mid * 6] <= i) lo = mid;
      else hi = mid - 1;
    }
    const int64_t* r = runs + lo * 6;
    int64_t k = i - r[0];
    if (r[2]) {  // literal bit-packed group
      int bit_width = (int)r[4];
      uint64_t mask = bit_width >= 32 ? 0xFFFFFFFFull : ((1ull << bit_width) - 1);
      uint64_t bitpos = (uint64_t)r[3] + (uint64_t)k * bit_width;
      uint64_t w;
      __builtin_memcpy(&w, payload + (bitpos >> 3), 8);
      out[i] = (int32_t)(((w >> (bitpos & 7)) & mask) + (uint64_t)r[5]);
    } else {
      out[i] = (int32_t)r[3];
    }
  }
}

// dictionary gather + validity scatter fused.
// positions: exclusive-scan of validity (dense index per valid row);
// validity==nullptr means all valid and positions==nullptr.
template <typename T>
__global__ void dict_gather_scatter_kernel(const T* __restrict__ dict,
                                           const int32_t* __restrict__ idx,
                                           const uint8_t* __restrict__ validity,
                                           const int64_t* __restrict__ positions,
                                           T* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (validity) {
      out[i] = validity[i] ? dict[idx[positions[i]]] : (T)0;
    } else {
      out[i] = dict[idx[i]];
    }
  }
}

// dense -> full-length scatter through validity (PLAIN nullable columns)
template <typename T>
__global__ void scatter_valid_kernel(const T* __restrict__ dense,
                                     const uint8_t* __restrict__ validity,
                                     const int64_t* __restrict__ positions,
                                     T* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    out[i] = validity[i] ? dense[positions[i]] : (T)0;
  }
}

// ===================================================================== //
// batched merge-path rounds (keys u64 + row index i64)
// ===================================================================== //
// One launch merges every pair of a round (MergeTable, kernels.h; the
// plan: ../cpp/merge_plan.h). A is the OLDER stream of a pair: on equal
// keys A's elements are emitted first so the newest row survives
// dedup-keep-last (UseLast semantics, reference sorted_stream_merger.rs /
// combiner.rs).

#define MERGE_VT 8
#define MERGE_TILE (LS_THREADS * MERGE_VT)  // 2048
static_assert(MERGE_TILE == MERGE_TILE_ROWS, "tile size of the host plan");

// key i of a stream as an order-preserving u64. Input streams (raw) hold
// keys in the launch's format KF, every other stream packed keys.
template <int KF>
__device__ inline uint64_t merge_load_key(const void* k, bool raw, int64_t i) {
  if constexpr (KF == MERGE_KEY_I64) {
    if (raw) return (uint64_t)((const int64_t*)k)[i] ^ 0x8000000000000000ull;
  } else if constexpr (KF == MERGE_KEY_I32) {
    if (raw) return (uint64_t)((uint32_t)((const int32_t*)k)[i] ^ 0x80000000u);
  }
  return ((const uint64_t*)k)[i];
}

// merge-path split of diagonal d: how many of the first d merged elements
// come from A. The whole wave searches: each pass probes 64 split points,
// so ~4 dependent loads find a split among 2^24 where a binary search
// needs 24. Every lane of the wave must call it with the same arguments;
// all lanes return the split.
template <int KF>
__device__ inline int64_t merge_path_search_wave(const void* A, bool rawA, int64_t nA,
                                                 const void* B, bool rawB, int64_t nB,
                                                 int64_t d, int lane) {
  int64_t lo = d > nB ? d - nB : 0;
  int64_t hi = d < nA ? d : nA;
  // invariant: pred(mid) = A[mid] <= B[d-mid-1] holds below the split and
  // fails from it on; lo <= split <= hi
  while (lo < hi) {
    int64_t span = hi - lo;
    int64_t mid = lo + ((span * lane) >> 6);  // in [lo, hi), lane 0 at lo
    bool pred = merge_load_key<KF>(A, rawA, mid) <= merge_load_key<KF>(B, rawB, d - mid - 1);
    int c = __popcll(__ballot(pred));  // lanes 0..c-1 hold, lane c fails
    int64_t nlo = c > 0 ? lo + ((span * (c - 1)) >> 6) + 1 : lo;
    int64_t nhi = c < 64 ? lo + ((span * c) >> 6) : hi;
    lo = nlo;
    hi = nhi;
  }
  return lo;
}

// KEEP_LAST = false: a merge round, keys and rows out.
// KEEP_LAST = true: the last round of a UseLast merge (one pair): no keys
// out; a row survives when its successor in merged order has another key.
template <int KF, bool KEEP_LAST>
__global__ __launch_bounds__(LS_THREADS) void merge_round_kernel(MergeTable tbl) {
  // A window then B window (KEEP_LAST: each one element longer where the
  // stream goes on, for the successor of the tile's last row); after the
  // merge the same arrays stage the tile's output. +4: the heads read one
  // past a window's end before the bounds are checked.
  __shared__ uint64_t sk[MERGE_TILE + 4];
  __shared__ int64_t sv[MERGE_TILE + 4];
  __shared__ int64_t s_bounds[2];
  __shared__ int s_wave_kept[LS_THREADS / 64];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t tile = blockIdx.x; tile < tbl.ntiles; tile += gridDim.x) {
    int j = 0;
    while (j + 1 < tbl.npairs && tbl.p[j + 1].first_tile <= tile) j++;
    const void* kA = tbl.p[j].kA;
    const void* kB = tbl.p[j].kB;
    const int64_t* rA = tbl.p[j].rA;
    const int64_t* rB = tbl.p[j].rB;
    const int64_t nA = tbl.p[j].nA, nB = tbl.p[j].nB;
    const bool rawA = rA == nullptr, rawB = rB == nullptr;
    const int64_t total = nA + nB;
    const int64_t d0 = (tile - tbl.p[j].first_tile) * MERGE_TILE;
    const int64_t d1 = d0 + MERGE_TILE < total ? d0 + MERGE_TILE : total;

    // waves 0 and 1 find the tile's two splits side by side
    if (wave < 2) {
      int64_t a = merge_path_search_wave<KF>(kA, rawA, nA, kB, rawB, nB,
                                             wave ? d1 : d0, lane);
      if (lane == 0) s_bounds[wave] = a;
    }
    __syncthreads();
    const int64_t a0 = s_bounds[0], a1 = s_bounds[1];
    const int64_t b0 = d0 - a0, b1 = d1 - a1;
    const int aCount = (int)(a1 - a0), bCount = (int)(b1 - b0);
    const int aExt = aCount + ((KEEP_LAST && a1 < nA) ? 1 : 0);
    const int bExt = bCount + ((KEEP_LAST && b1 < nB) ? 1 : 0);

    // stage keys and rows: [0, aExt) = A, [aExt, aExt + bExt) = B
    for (int i = threadIdx.x; i < aExt; i += LS_THREADS) {
      sk[i] = merge_load_key<KF>(kA, rawA, a0 + i);
      sv[i] = rawA ? tbl.p[j].baseA + a0 + i : rA[a0 + i];
    }
    for (int i = threadIdx.x; i < bExt; i += LS_THREADS) {
      sk[aExt + i] = merge_load_key<KF>(kB, rawB, b0 + i);
      sv[aExt + i] = rawB ? tbl.p[j].baseB + b0 + i : rB[b0 + i];
    }
    __syncthreads();

    // each thread merges MERGE_VT outputs starting at its local diagonal
    const int out_n = (int)(d1 - d0);
    const int local_d = threadIdx.x * MERGE_VT;
    int count = out_n - local_d;
    count = count < 0 ? 0 : count > MERGE_VT ? MERGE_VT : count;
    uint64_t ok[MERGE_VT];
    int64_t ov[MERGE_VT];
    int ai = 0, bi = 0;
    if (count) {
      int lo = local_d > bCount ? local_d - bCount : 0;
      int hi = local_d < aCount ? local_d : aCount;
      while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (sk[mid] <= sk[aExt + local_d - mid - 1]) lo = mid + 1;
        else hi = mid;
      }
      ai = lo;
      bi = local_d - lo;
    }
    uint64_t ka = sk[ai], kb = sk[aExt + bi];
    int64_t va = sv[ai], vb = sv[aExt + bi];
#pragma unroll
    for (int k = 0; k < MERGE_VT; k++) {
      if (k < count) {
        bool takeA = bi >= bCount || (ai < aCount && ka <= kb);
        if (takeA) {
          ok[k] = ka;
          ov[k] = va;
          ai++;
          ka = sk[ai];
          va = sv[ai];
        } else {
          ok[k] = kb;
          ov[k] = vb;
          bi++;
          kb = sk[aExt + bi];
          vb = sv[aExt + bi];
        }
      }
    }

    if constexpr (!KEEP_LAST) {
      __syncthreads();  // every thread is done with the windows
#pragma unroll
      for (int k = 0; k < MERGE_VT; k++) {
        if (k < count) {
          sk[local_d + k] = ok[k];
          sv[local_d + k] = ov[k];
        }
      }
      __syncthreads();
      uint64_t* kOut = tbl.p[j].kOut + d0;
      int64_t* rOut = tbl.p[j].rOut + d0;
      for (int i = threadIdx.x; i < out_n; i += LS_THREADS) {
        kOut[i] = sk[i];
        rOut[i] = sv[i];
      }
    } else {
      // the successor of this thread's last row is the smaller head left
      // (ka, kb): inside the tile, or the element after the window. No
      // head left: the last row of all, which is kept.
      const bool hasA = ai < aExt, hasB = bi < bExt;
      const uint64_t succ = hasA && hasB ? (ka <= kb ? ka : kb) : hasA ? ka : kb;
      const bool has_succ = hasA || hasB;
      unsigned keep = 0;
#pragma unroll
      for (int k = 0; k < MERGE_VT; k++) {
        if (k < count) {
          bool kp = k + 1 < count ? ok[k] != ok[k + 1] : (!has_succ || ok[k] != succ);
          keep |= (unsigned)kp << k;
        }
      }
      // exclusive scan of the kept counts over the workgroup
      const int mine = __popc(keep);
      int incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
      }
      if (lane == 63) s_wave_kept[wave] = incl;
      __syncthreads();  // also: every thread is done with the windows
      int pos = incl - mine, tile_kept = 0;
#pragma unroll
      for (int w = 0; w < LS_THREADS / 64; w++) {
        if (w < wave) pos += s_wave_kept[w];
        tile_kept += s_wave_kept[w];
      }
#pragma unroll
      for (int k = 0; k < MERGE_VT; k++) {
        if (keep >> k & 1) sv[pos++] = ov[k];
      }
      __syncthreads();
      int64_t* slot = tbl.p[j].rOut + d0;
      for (int i = threadIdx.x; i < tile_kept; i += LS_THREADS) slot[i] = sv[i];
      if (threadIdx.x == 0) tbl.tile_counts[tile] = tile_kept;
    }
    __syncthreads();  // the next tile reuses the arrays
  }
}

// moves the survivors of every tile of the keep-last round to their place
__global__ void compact_tiles_kernel(const int64_t* __restrict__ slots,
                                     const int64_t* __restrict__ counts,
                                     const int64_t* __restrict__ csum,
                                     int64_t ntiles, int64_t* __restrict__ out) {
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int64_t cnt = counts[tile];
    const int64_t* src = slots + tile * MERGE_TILE;
    int64_t* dst = out + (csum[tile] - cnt);
    for (int64_t i = threadIdx.x; i < cnt; i += blockDim.x) dst[i] = src[i];
  }
}

// group-start mask: start[i] = (i==0) || key[i] != key[i-1]
__global__ void group_start_mask_kernel(const uint64_t* __restrict__ keys,
                                        uint8_t* __restrict__ start, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    start[i] = (i == 0) || (keys[i] != keys[i - 1]);
  }
}

// order-preserving u64 key packing
__global__ void pack_key_i64_kernel(const int64_t* __restrict__ x,
                                    uint64_t* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    out[i] = (uint64_t)x[i] ^ 0x8000000000000000ull;
  }
}

__global__ void pack_key_2xi32_kernel(const int32_t* __restrict__ hi,
                                      const int32_t* __restrict__ lo,
                                      uint64_t* __restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint64_t h = (uint32_t)hi[i] ^ 0x80000000u;
    uint64_t l = (uint32_t)lo[i] ^ 0x80000000u;
    out[i] = (h << 32) | l;
  }
}

// ===================================================================== //
// gather kernels (payload materialization after merge)
// ===================================================================== //

// fused multi-column fixed-width gather: up to 16 columns per launch.
// srcs/dsts are device pointer tables; elem sizes per column
// (struct GatherTable, kernels.h).
__global__ void gather_fixed_multi_kernel(GatherTable tbl,
                                          const int64_t* __restrict__ idx,
                                          int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t s = idx[i];
#pragma unroll 4
    for (int c = 0; c < tbl.ncols; c++) {
      switch (tbl.esize[c]) {
        case 1: ((uint8_t*)tbl.dst[c])[i] = ((const uint8_t*)tbl.src[c])[s]; break;
        case 2: ((uint16_t*)tbl.dst[c])[i] = ((const uint16_t*)tbl.src[c])[s]; break;
        case 4: ((uint32_t*)tbl.dst[c])[i] = ((const uint32_t*)tbl.src[c])[s]; break;
        default: ((uint64_t*)tbl.dst[c])[i] = ((const uint64_t*)tbl.src[c])[s]; break;
      }
    }
  }
}

// the same gather straight from the per-file buffers of a scan unit
// (struct GatherFilesTable, kernels.h): no concatenated copy of the
// columns is made first. The file of a row is found by counting the row
// starts at or below it (an upper bound over <= 16 entries held in LDS).
__global__ __launch_bounds__(LS_THREADS) void gather_files_kernel(
    GatherFilesTable tbl, const int64_t* __restrict__ idx, int64_t n) {
  __shared__ const void* s_src[GATHER_FILES_MAX_COLS * GATHER_FILES_MAX_FILES];
  __shared__ int64_t s_start[GATHER_FILES_MAX_FILES + 1];
  for (int i = threadIdx.x; i < GATHER_FILES_MAX_COLS * GATHER_FILES_MAX_FILES;
       i += LS_THREADS)
    s_src[i] = tbl.src[i / GATHER_FILES_MAX_FILES][i % GATHER_FILES_MAX_FILES];
  if (threadIdx.x <= GATHER_FILES_MAX_FILES) s_start[threadIdx.x] = tbl.start[threadIdx.x];
  __syncthreads();
  const int nfiles = tbl.nfiles;
  const int64_t lo = tbl.start[0], hi = tbl.start[nfiles];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t s = idx[i];
    if (s < lo || s >= hi) continue;
    int f = 0;
    for (int j = 1; j < nfiles; j++) f += s_start[j] <= s;
    int64_t r = s - s_start[f];
    for (int c = 0; c < tbl.ncols; c++) {
      const void* p = s_src[c * GATHER_FILES_MAX_FILES + f];
      switch (tbl.esize[c]) {
        case 1: ((uint8_t*)tbl.dst[c])[i] = p ? ((const uint8_t*)p)[r] : (uint8_t)1; break;
        case 2: ((uint16_t*)tbl.dst[c])[i] = p ? ((const uint16_t*)p)[r] : (uint16_t)1; break;
        case 4: ((uint32_t*)tbl.dst[c])[i] = p ? ((const uint32_t*)p)[r] : 1u; break;
        default: ((uint64_t*)tbl.dst[c])[i] = p ? ((const uint64_t*)p)[r] : 1ull; break;
      }
    }
  }
}

// string gather: one wave per output row; lanes copy bytes cooperatively.
__global__ void gather_strings_kernel(const uint8_t* __restrict__ src_bytes,
                                      const int64_t* __restrict__ src_offsets,
                                      const int64_t* __restrict__ idx,
                                      const int64_t* __restrict__ dst_offsets,
                                      uint8_t* __restrict__ dst_bytes,
                                      int64_t n) {
  int64_t waves_per_grid = ((int64_t)gridDim.x * blockDim.x) >> 6;
  int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  int lane = threadIdx.x & 63;
  for (int64_t i = wave; i < n; i += waves_per_grid) {
    int64_t s = idx[i];
    int64_t so = src_offsets[s], eo = src_offsets[s + 1];
    int64_t d = dst_offsets[i];
    for (int64_t b = lane; b < eo - so; b += 64) {
      dst_bytes[d + b] = src_bytes[so + b];
    }
  }
}

// CDC filter: mask[i] = (value != pattern)
__global__ void bytes_ne_mask_kernel(const int64_t* __restrict__ offsets,
                                     const uint8_t* __restrict__ bytes,
                                     const uint8_t* __restrict__ pattern,
                                     int plen, uint8_t* __restrict__ out,
                                     int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t so = offsets[i], eo = offsets[i + 1];
    bool eq = (eo - so) == plen;
    if (eq) {
      for (int k = 0; k < plen; k++) {
        if (bytes[so + k] != pattern[k]) {
          eq = false;
          break;
        }
      }
    }
    out[i] = eq ? 0 : 1;
  }
}

// segmented sum over sorted groups: starts-based two-phase not needed —
// use atomics into per-group slot (group ids from scan of start mask).
__device__ inline void ls_atomic_add(float* p, float v) { atomicAdd(p, v); }
__device__ inline void ls_atomic_add(double* p, double v) { atomicAdd(p, v); }
__device__ inline void ls_atomic_add(int32_t* p, int32_t v) { atomicAdd(p, v); }
__device__ inline void ls_atomic_add(int64_t* p, int64_t v) {
  atomicAdd((unsigned long long*)p, (unsigned long long)v);
}

template <typename T, typename ACC>
__global__ void segmented_sum_kernel(const T* __restrict__ vals,
                                     const int64_t* __restrict__ group_of_row,
                                     const uint8_t* __restrict__ contrib,
                                     const uint8_t* __restrict__ validity,
                                     ACC* __restrict__ out_sum,
                                     int32_t* __restrict__ out_has_null,
                                     int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (contrib && !contrib[i]) continue;
    int64_t g = group_of_row[i];
    if (validity && !validity[i]) {
      out_has_null[g] = 1;
      continue;
    }
    ls_atomic_add(&out_sum[g], (ACC)vals[i]);
  }
}

// last contributing (and optionally non-null) row index per group.
// out_idx is zero-initialized and stores (i+1) — unsigned atomicMax can't
// start from -1 (0xFF..F would already be maximal). 0 means "no row".
__global__ void segmented_last_kernel(const int64_t* __restrict__ group_of_row,
                                      const uint8_t* __restrict__ contrib,
                                      const uint8_t* __restrict__ validity,
                                      int64_t* __restrict__ out_idx,  // init 0
                                      int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (contrib && !contrib[i]) continue;
    if (validity && !validity[i]) continue;
    atomicMax((unsigned long long*)&out_idx[group_of_row[i]],
              (unsigned long long)(i + 1));
  }
}

}  // namespace lakesoul

// ===================================================================== //
// host-side launchers (called from hip_module.cc)
// ===================================================================== //

namespace lakesoul {

void launch_hash_fixed(int dt, const void* data, const uint8_t* validity,
                       const int64_t* prev, int64_t* out, int64_t n, int first,
                       hipStream_t stream) {
  dim3 g(ls_blocks(n)), b(LS_THREADS);
  switch (dt) {
    case 0: hipLaunchKernelGGL((hash_fixed_kernel<0>), g, b, 0, stream, data, validity, prev, out, n, first); break;
    case 1: hipLaunchKernelGGL((hash_fixed_kernel<1>), g, b, 0, stream, data, validity, prev, out, n, first); break;
    case 2: hipLaunchKernelGGL((hash_fixed_kernel<2>), g, b, 0, stream, data, validity, prev, out, n, first); break;
    case 3: hipLaunchKernelGGL((hash_fixed_kernel<3>), g, b, 0, stream, data, validity, prev, out, n, first); break;
    case 4: hipLaunchKernelGGL((hash_fixed_kernel<4>), g, b, 0, stream, data, validity, prev, out, n, first); break;
    case 5: hipLaunchKernelGGL((hash_fixed_kernel<5>), g, b, 0, stream, data, validity, prev, out, n, first); break;
    default: hipLaunchKernelGGL((hash_fixed_kernel<6>), g, b, 0, stream, data, validity, prev, out, n, first); break;
  }
}

void launch_hash_string(const int32_t* offsets, const uint8_t* bytes,
                        const uint8_t* validity, const int64_t* prev,
                        int64_t* out, int64_t n, int first, hipStream_t s) {
  hipLaunchKernelGGL(hash_string_kernel, dim3(ls_blocks(n)), dim3(LS_THREADS), 0, s,
                     offsets, bytes, validity, prev, out, n, first);
}

void launch_bucket_ids(const int64_t* hashes, int32_t* out, int64_t n,
                       uint32_t nb, hipStream_t s) {
  hipLaunchKernelGGL(bucket_ids_kernel, dim3(ls_blocks(n)), dim3(LS_THREADS), 0, s,
                     hashes, out, n, nb);
}

void launch_rle_expand(const uint8_t* payload, const int64_t* runs,
                       int64_t nruns, int32_t* out, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(rle_expand_kernel, dim3(ls_blocks(n)), dim3(LS_THREADS), 0, s,
                     payload, runs, nruns, out, n);
}

template <typename T>
void launch_dict_gather_scatter(const T* dict, const int32_t* idx,
                                const uint8_t* validity, const int64_t* pos,
                                T* out, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL((dict_gather_scatter_kernel<T>), dim3(ls_blocks(n)),
                     dim3(LS_THREADS), 0, s, dict, idx, validity, pos, out, n);
}
template void launch_dict_gather_scatter<uint32_t>(const uint32_t*, const int32_t*, const uint8_t*, const int64_t*, uint32_t*, int64_t, hipStream_t);
template void launch_dict_gather_scatter<uint64_t>(const uint64_t*, const int32_t*, const uint8_t*, const int64_t*, uint64_t*, int64_t, hipStream_t);
template void launch_dict_gather_scatter<uint8_t>(const uint8_t*, const int32_t*, const uint8_t*, const int64_t*, uint8_t*, int64_t, hipStream_t);

template <typename T>
void launch_scatter_valid(const T* dense, const uint8_t* validity,
                          const int64_t* pos, T* out, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL((scatter_valid_kernel<T>), dim3(ls_blocks(n)),
                     dim3(LS_THREADS), 0, s, dense, validity, pos, out, n);
}
template void launch_scatter_valid<uint8_t>(const uint8_t*, const uint8_t*, const int64_t*, uint8_t*, int64_t, hipStream_t);
template void launch_scatter_valid<uint16_t>(const uint16_t*, const uint8_t*, const int64_t*, uint16_t*, int64_t, hipStream_t);
template void launch_scatter_valid<uint32_t>(const uint32_t*, const uint8_t*, const int64_t*, uint32_t*, int64_t, hipStream_t);
template void launch_scatter_valid<uint64_t>(const uint64_t*, const uint8_t*, const int64_t*, uint64_t*, int64_t, hipStream_t);

template <bool KEEP_LAST>
static void launch_merge_round_t(const MergeTable& tbl, int key_format, hipStream_t s) {
  if (tbl.ntiles <= 0) return;  // a grid of 0 blocks is an error
  dim3 g(tbl.ntiles > LS_MAX_BLOCKS ? LS_MAX_BLOCKS : (int)tbl.ntiles), b(LS_THREADS);
  switch (key_format) {
    case MERGE_KEY_I64: hipLaunchKernelGGL((merge_round_kernel<MERGE_KEY_I64, KEEP_LAST>), g, b, 0, s, tbl); break;
    case MERGE_KEY_I32: hipLaunchKernelGGL((merge_round_kernel<MERGE_KEY_I32, KEEP_LAST>), g, b, 0, s, tbl); break;
    default: hipLaunchKernelGGL((merge_round_kernel<MERGE_KEY_PACKED, KEEP_LAST>), g, b, 0, s, tbl); break;
  }
}

void launch_merge_round(const MergeTable& tbl, int key_format, hipStream_t s) {
  launch_merge_round_t<false>(tbl, key_format, s);
}

void launch_merge_round_keep_last(const MergeTable& tbl, int key_format,
                                  hipStream_t s) {
  launch_merge_round_t<true>(tbl, key_format, s);
}

void launch_compact_tiles(const int64_t* slots, const int64_t* counts,
                          const int64_t* csum, int64_t ntiles, int64_t* out,
                          hipStream_t s) {
  if (ntiles <= 0) return;
  hipLaunchKernelGGL(compact_tiles_kernel,
                     dim3(ntiles > LS_MAX_BLOCKS ? LS_MAX_BLOCKS : (int)ntiles),
                     dim3(LS_THREADS), 0, s, slots, counts, csum, ntiles, out);
}

void launch_group_start(const uint64_t* keys, uint8_t* start, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(group_start_mask_kernel, dim3(ls_blocks(n)), dim3(LS_THREADS), 0, s,
                     keys, start, n);
}

void launch_pack_key_i64(const int64_t* x, uint64_t* out, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(pack_key_i64_kernel, dim3(ls_blocks(n)), dim3(LS_THREADS), 0, s,
                     x, out, n);
}

void launch_pack_key_2xi32(const int32_t* hi, const int32_t* lo, uint64_t* out,
                           int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(pack_key_2xi32_kernel, dim3(ls_blocks(n)), dim3(LS_THREADS), 0, s,
                     hi, lo, out, n);
}

void launch_gather_fixed_multi(const GatherTable& tbl, const int64_t* idx,
                               int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(gather_fixed_multi_kernel, dim3(ls_blocks(n)),
                     dim3(LS_THREADS), 0, s, tbl, idx, n);
}

void launch_gather_files(const GatherFilesTable& tbl, const int64_t* idx,
                         int64_t n, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(gather_files_kernel, dim3(ls_blocks(n)), dim3(LS_THREADS),
                     0, s, tbl, idx, n);
}

void launch_gather_strings(const uint8_t* src_bytes, const int64_t* src_off,
                           const int64_t* idx, const int64_t* dst_off,
                           uint8_t* dst_bytes, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(gather_strings_kernel, dim3(ls_blocks(n, 1)),
                     dim3(LS_THREADS), 0, s, src_bytes, src_off, idx, dst_off,
                     dst_bytes, n);
}

void launch_bytes_ne_mask(const int64_t* offsets, const uint8_t* bytes,
                          const uint8_t* pattern, int plen, uint8_t* out,
                          int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(bytes_ne_mask_kernel, dim3(ls_blocks(n)), dim3(LS_THREADS),
                     0, s, offsets, bytes, pattern, plen, out, n);
}

template <typename T, typename ACC>
void launch_segmented_sum(const T* vals, const int64_t* grp, const uint8_t* contrib,
                          const uint8_t* validity, ACC* out_sum,
                          int32_t* out_has_null, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL((segmented_sum_kernel<T, ACC>), dim3(ls_blocks(n)),
                     dim3(LS_THREADS), 0, s, vals, grp, contrib, validity,
                     out_sum, out_has_null, n);
}
template void launch_segmented_sum<float, float>(const float*, const int64_t*, const uint8_t*, const uint8_t*, float*, int32_t*, int64_t, hipStream_t);
template void launch_segmented_sum<double, double>(const double*, const int64_t*, const uint8_t*, const uint8_t*, double*, int32_t*, int64_t, hipStream_t);
template void launch_segmented_sum<int32_t, int32_t>(const int32_t*, const int64_t*, const uint8_t*, const uint8_t*, int32_t*, int32_t*, int64_t, hipStream_t);
template void launch_segmented_sum<int64_t, int64_t>(const int64_t*, const int64_t*, const uint8_t*, const uint8_t*, int64_t*, int32_t*, int64_t, hipStream_t);

void launch_segmented_last(const int64_t* grp, const uint8_t* contrib,
                           const uint8_t* validity, int64_t* out_idx, int64_t n,
                           hipStream_t s) {
  hipLaunchKernelGGL(segmented_last_kernel, dim3(ls_blocks(n)), dim3(LS_THREADS),
                     0, s, grp, contrib, validity, out_idx, n);
}

}  // namespace lakesoul
namespace lakesoul {

// ------------------------------------------------------------------ //
// binary-code hamming scorer (vector index first pass — the RaBitQ
// 1-bit idea, lakesoul-vector quantizer.rs): codes are sign bits of
// rotated vectors packed into u64 words. Each thread owns one database
// row, keeps its W<=16 words in registers, loops the query block —
// codes read once from HBM per launch.
// ------------------------------------------------------------------ //

__global__ void hamming_scores_kernel(const uint64_t* __restrict__ codes,
                                      const uint64_t* __restrict__ qcodes,
                                      int32_t* __restrict__ out, int64_t n,
                                      int nq, int words) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  uint64_t c[16];
  for (; i < n; i += stride) {
    for (int w = 0; w < words; w++) c[w] = codes[i * words + w];
    for (int q = 0; q < nq; q++) {
      int d = 0;
      for (int w = 0; w < words; w++)
        d += __popcll(c[w] ^ qcodes[q * words + w]);
      out[i * nq + q] = d;
    }
  }
}

// 8-byte big-endian chunk key of each string (zero-padded past the
// end), sign-flipped so int64 ascending sort = unsigned byte order.
// LSD passes over chunks + a length pass give full lexicographic order
// on the GPU (string-PK merge; reference cursors compare byte-wise,
// sorted/cursor.rs).
__global__ void str_chunk_keys_kernel(const int64_t* __restrict__ offsets,
                                      const uint8_t* __restrict__ bytes,
                                      int64_t chunk, int64_t* __restrict__ out,
                                      int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    int64_t a = offsets[i], b = offsets[i + 1];
    int64_t start = a + chunk * 8;
    uint64_t key = 0;
    for (int k = 0; k < 8; k++) {
      uint64_t v = (start + k < b) ? bytes[start + k] : 0;
      key = (key << 8) | v;
    }
    out[i] = (int64_t)(key ^ 0x8000000000000000ull);
  }
}

void launch_str_chunk_keys(const int64_t* offsets, const uint8_t* bytes,
                           int64_t chunk, int64_t* out, int64_t n,
                           hipStream_t s) {
  hipLaunchKernelGGL(str_chunk_keys_kernel, dim3(ls_blocks(n)),
                     dim3(LS_THREADS), 0, s, offsets, bytes, chunk, out, n);
}

void launch_hamming_scores(const uint64_t* codes, const uint64_t* qcodes,
                           int32_t* out, int64_t n, int nq, int words,
                           hipStream_t s) {
  hipLaunchKernelGGL(hamming_scores_kernel, dim3(ls_blocks(n)), dim3(LS_THREADS),
                     0, s, codes, qcodes, out, n, nq, words);
}

}  // namespace lakesoul
