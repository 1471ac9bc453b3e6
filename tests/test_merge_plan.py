"""The host plan of the batched merge rounds (csrc/cpp/merge_plan.h, through
_cpp.merge_plan): pairing in input order, tile prefix, output ranges, the
carried stream and the scratch buffers, for 1 to 40 streams of lengths
around the 2048-row tile. No GPU."""

import math

import numpy as np
import pytest

LENS = [0, 1, 2047, 2048, 2049, 5, 4100]


def _plan(lens):
    from lakesoul_amd.ops import cpp

    return cpp().merge_plan([int(x) for x in lens])


def _cases():
    rng = np.random.default_rng(7)
    for k in range(1, 41):
        yield [LENS[(i + k) % len(LENS)] for i in range(k)]
        yield [int(x) for x in rng.choice(LENS, k)]
    yield [0] * 5
    yield [2048] * 16
    yield [0, 2048, 0]


def _check(lens):
    rounds, nbufs, n, tile = _plan(lens)
    k = len(lens)
    starts = np.concatenate([[0], np.cumsum(lens)])
    assert tile == 2048 and n == starts[-1]
    assert len(rounds) == (math.ceil(math.log2(k)) if k > 1 else 0)
    # the streams a round reads: (buf, first, count, off, n)
    cur = [(-1, i, 1, int(starts[i]), int(lens[i])) for i in range(k)]
    used_bufs = set()
    for ri, (pairs, carry, buf_out, ntiles) in enumerate(rounds):
        last = ri == len(rounds) - 1
        assert len(pairs) == len(cur) // 2
        assert buf_out == (-2 if last else buf_out) and (last or 0 <= buf_out < nbufs)
        nxt, tiles_seen, out_ranges = [], 0, []
        for j, (a, b, first_tile, pt) in enumerate(pairs):
            # pairing in input order; a is the older stream
            assert a == cur[2 * j] and b == cur[2 * j + 1]
            assert a[3] + a[4] == b[3] and a[1] + a[2] == b[1]
            # every tile belongs to exactly one pair: the pairs' tile ranges
            # follow each other without gap or overlap
            assert first_tile == tiles_seen
            assert pt == -(-(a[4] + b[4]) // tile)
            tiles_seen += pt
            # a pair never writes the buffer one of its inputs lives in
            assert last or (a[0] != buf_out and b[0] != buf_out)
            out_ranges.append((a[3], a[3] + a[4] + b[4]))
            nxt.append((buf_out, a[1], a[2] + b[2], a[3], a[4] + b[4]))
        assert tiles_seen == ntiles
        if len(cur) % 2:
            # the carried stream is the last one, kept where it is
            assert carry == cur[-1]
            out_ranges.append((carry[3], carry[3] + carry[4]))
            nxt.append(carry)
        else:
            assert carry is None
        # the output ranges (and the carried stream) partition [0, n)
        pos = 0
        for lo, hi in out_ranges:
            assert lo == pos and hi >= lo
            pos = hi
        assert pos == n
        if not last:
            used_bufs.add(buf_out)
        cur = nxt
    if k > 1:
        assert cur == [(-2, 0, k, 0, n)]
    assert nbufs == len(used_bufs) <= 3


@pytest.mark.parametrize("case", list(_cases()), ids=lambda c: f"k{len(c)}-{sum(c)}")
def test_merge_plan(case):
    _check(case)


def test_merge_plan_buffers():
    """Two scratch buffers ping-pong for the benchmark's 11 files and up to
    13 streams; at 14 a pair reads a carried stream from the buffer whose
    turn it would be, and the plan takes a third."""
    for k in range(1, 14):
        assert _plan([100] * k)[1] <= 2
    assert _plan([3000] + [600] * 10)[1] == 2
    assert _plan([100] * 14)[1] == 3
