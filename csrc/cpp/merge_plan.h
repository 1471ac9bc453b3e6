// Host plan of the batched pairwise merge (csrc/hip/kernels.hip,
// merge_round_kernel): k sorted streams are merged in ceil(log2(k)) rounds;
// one round merges every pair of neighbouring streams, in input order, and
// is one kernel launch (per MERGE_PAIRS_PER_LAUNCH pairs). Plain C++, no
// GPU: the stream lengths alone fix the whole plan.
//
// Positions. A stream of a round is a run of consecutive input streams, so
// it starts at `off` = the number of rows of all inputs before it, in every
// round; a pair's output starts where its A stream starts. The streams of a
// round therefore partition [0, n) and each buffer is indexed by position.
//
// Buffers. `buf` says where a stream lives: MP_INPUT (stream `first` of the
// caller's inputs, keys still in the caller's format, row value = off + i,
// never stored) or a scratch buffer 0, 1, 2 holding packed keys and row
// values at [off, off + n). An odd last stream is carried to the next round
// by keeping its (buf, off): nothing is copied, and no pair of the round
// writes its range. A round writes the lowest scratch buffer that none of
// its pairs reads. Two buffers ping-pong unless a pair reads a carried
// stream out of the buffer that would be written (first at 14 streams);
// `nbufs` says how many the plan uses. The last round is written to the
// caller's result (buf_out = MP_RESULT).
#pragma once

#include <cstdint>
#include <vector>

namespace lakesoul {

constexpr int64_t MERGE_TILE_ROWS = 2048;  // outputs per workgroup tile
constexpr int MP_INPUT = -1;
constexpr int MP_RESULT = -2;

struct MergeStream {
  int buf = MP_INPUT;  // MP_INPUT or scratch buffer id
  int first = 0;       // first input stream this one covers
  int count = 1;       // how many input streams it covers
  int64_t off = 0;     // rows of all inputs before it
  int64_t n = 0;       // its rows
};

struct MergePair {
  MergeStream a, b;        // a is the older stream: first on equal keys
  int64_t first_tile = 0;  // tiles of this round before this pair
  int64_t ntiles = 0;      // ceil((a.n + b.n) / MERGE_TILE_ROWS)
  // output: [a.off, a.off + a.n + b.n) of the round's buf_out
};

struct MergeRound {
  std::vector<MergePair> pairs;
  bool has_carry = false;
  MergeStream carry;  // the last stream, when the round has an odd number
  int buf_out = 0;    // scratch buffer id, or MP_RESULT in the last round
  int64_t ntiles = 0;
};

struct MergePlan {
  std::vector<MergeRound> rounds;  // empty for one stream
  int nbufs = 0;                   // scratch buffers used (0..3)
  int64_t n = 0;                   // rows of all streams
};

inline MergePlan plan_merge(const std::vector<int64_t>& lens) {
  MergePlan plan;
  std::vector<MergeStream> cur;
  for (size_t i = 0; i < lens.size(); i++) {
    MergeStream s;
    s.first = (int)i;
    s.off = plan.n;
    s.n = lens[i];
    plan.n += lens[i];
    cur.push_back(s);
  }
  while (cur.size() > 1) {
    MergeRound r;
    bool last = cur.size() == 2;
    if (last) {
      r.buf_out = MP_RESULT;
    } else {
      bool used[3] = {false, false, false};
      // the carried stream is not read now, and no pair writes its range
      for (size_t j = 0; j < cur.size() - cur.size() % 2; j++)
        if (cur[j].buf >= 0) used[cur[j].buf] = true;
      r.buf_out = !used[0] ? 0 : !used[1] ? 1 : 2;
      if (r.buf_out + 1 > plan.nbufs) plan.nbufs = r.buf_out + 1;
    }
    std::vector<MergeStream> next;
    for (size_t j = 0; j + 1 < cur.size(); j += 2) {
      MergePair p;
      p.a = cur[j];
      p.b = cur[j + 1];
      p.first_tile = r.ntiles;
      p.ntiles = (p.a.n + p.b.n + MERGE_TILE_ROWS - 1) / MERGE_TILE_ROWS;
      r.ntiles += p.ntiles;
      r.pairs.push_back(p);
      MergeStream o;
      o.buf = r.buf_out;
      o.first = p.a.first;
      o.count = p.a.count + p.b.count;
      o.off = p.a.off;
      o.n = p.a.n + p.b.n;
      next.push_back(o);
    }
    if (cur.size() % 2) {
      r.has_carry = true;
      r.carry = cur.back();
      next.push_back(cur.back());
    }
    plan.rounds.push_back(std::move(r));
    cur = std::move(next);
  }
  return plan;
}

}  // namespace lakesoul
