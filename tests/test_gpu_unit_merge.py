"""The unit merge kernels directly (csrc/hip/kernels.hip): the batched merge
rounds with the fused keep-last round (_hip.unit_merge_src_idx), the same
rounds with keys out (_hip.merge_sorted_keys) and the gather from per-file
buffers (_hip.gather_files), each against a few lines of numpy: concatenate,
stable argsort, keep the last row of every run of equal keys.

Sizes sit around the 2048-row merge tile, the 16-pair launch table (33
streams), the 16-file gather table, and once past the 2048-block grid cap."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 2048

# stream lengths: one stream of each edge length, two and three streams
# (odd carry), an empty stream between full ones, the benchmark's 11 files,
# 33 streams (17 pairs: two launches in the first round; a third scratch
# buffer), 14 streams (a carried stream read from a scratch buffer)
SHAPES = (
    [[n] for n in (0, 1, 2047, 2048, 2049)]
    + [[2049, 2047], [1, 0], [0, 0], [2048, 2048]]
    + [[2047, 1, 2049], [2048, 0, 2048], [0, 5, 0]]
    + [[3000] + [600] * 10]
    + [[(37 * i) % 301 for i in range(33)]]
    + [[500 + i for i in range(14)]]
)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests require an MI355X"
    return torch.device("cuda:0")


def _ids(shape):
    return f"k{len(shape)}-n{sum(shape)}"


def _streams(rng, lens, dtype, ndistinct):
    """Sorted streams over a pool of `ndistinct` keys that holds both ends
    of the type, negatives and zero; drawn with replacement, so keys repeat
    inside a stream and across streams."""
    info = np.iinfo(dtype)
    pool = np.unique(np.concatenate([
        np.array([info.min, info.min + 1, -2, -1, 0, 1, info.max - 1, info.max],
                 dtype=dtype),
        rng.integers(info.min, info.max, max(ndistinct - 8, 1), dtype=dtype,
                     endpoint=True)]))
    return [np.sort(rng.choice(pool, n)).astype(dtype) for n in lens]


def _want(streams):
    """(sorted keys, order, src_idx) of the stable merge."""
    concat = np.concatenate(streams) if streams else np.zeros(0, np.int64)
    order = np.argsort(concat, kind="stable")
    keys = concat[order]
    keep = np.ones(len(keys), dtype=bool)
    keep[:-1] = keys[:-1] != keys[1:]
    return keys, order, order[keep]


def _src_idx(dev, streams):
    from lakesoul_amd.ops import hip

    out = hip().unit_merge_src_idx([torch.from_numpy(s).to(dev) for s in streams])
    assert out.dtype == torch.int64
    return out.cpu().numpy()


@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("lens", SHAPES, ids=_ids)
def test_src_idx_shapes(dev, lens, dtype):
    """Every shape with few distinct keys (long runs of equal keys inside
    and across streams, over tile edges) and with many."""
    rng = np.random.default_rng(len(lens) * 1000 + sum(lens))
    for ndistinct in (12, 4000):
        streams = _streams(rng, lens, dtype, ndistinct)
        np.testing.assert_array_equal(_src_idx(dev, streams), _want(streams)[2])


@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=["i64", "i32"])
def test_src_idx_all_equal(dev, dtype):
    """One key in every row of 11 streams: one run spans every tile, every
    tile but the last keeps nothing, and the survivor is the last row of
    the last stream."""
    lens = [3000] + [600] * 10
    for key in (np.iinfo(dtype).min, -1, np.iinfo(dtype).max):
        streams = [np.full(n, key, dtype=dtype) for n in lens]
        got = _src_idx(dev, streams)
        np.testing.assert_array_equal(got, [sum(lens) - 1])


def test_src_idx_run_over_tile_edge(dev):
    """Distinct keys but for one run of 40 equal keys, 20 in each stream,
    placed across the first tile edge of the last round; then the same with
    the run ending exactly at the edge."""
    for run_start in (TILE - 25, TILE - 40):
        a = np.arange(0, 6000, 2, dtype=np.int64)   # even keys
        b = np.arange(1, 6001, 2, dtype=np.int64)   # odd keys
        # merged position of key k is k: the run takes positions
        # run_start .. run_start + 39
        k0 = run_start
        a[(a >= k0) & (a < k0 + 40)] = k0
        b[(b >= k0) & (b < k0 + 40)] = k0
        streams = [np.sort(a), np.sort(b)]
        keys, _, want = _want(streams)
        assert (keys[run_start:run_start + 40] == k0).all()
        np.testing.assert_array_equal(_src_idx(dev, streams), want)


def test_src_idx_grid_stride(dev):
    """2048 tiles and 5000 rows more: the grid cap is 2048 blocks, so blocks
    take a second tile in both kernels of the last round."""
    total = TILE * 2048 + 5000
    rng = np.random.default_rng(5)
    na = total * 3 // 5
    streams = [np.sort(rng.integers(-2 ** 40, 2 ** 40, m)) for m in (na, total - na)]
    streams[1][::3] = streams[0][: len(streams[1][::3])]
    streams[1].sort()
    np.testing.assert_array_equal(_src_idx(dev, streams), _want(streams)[2])


@pytest.mark.parametrize("lens", SHAPES, ids=_ids)
def test_merge_sorted_keys_shapes(dev, lens):
    """merge_sorted_keys runs on the same rounds, packed keys in, keys and
    order out."""
    from lakesoul_amd.ops import hip

    rng = np.random.default_rng(len(lens) * 77 + sum(lens))
    for ndistinct in (12, 4000):
        # packed keys: any int64 bit pattern, ordered as unsigned
        streams = [np.sort(s.view(np.uint64)).view(np.int64)
                   for s in _streams(rng, lens, np.int64, ndistinct)]
        keys, order = hip().merge_sorted_keys(
            [torch.from_numpy(s).to(dev) for s in streams])
        wk, wo, _ = _want([s.view(np.uint64) for s in streams])
        np.testing.assert_array_equal(order.cpu().numpy(), wo)
        np.testing.assert_array_equal(keys.cpu().numpy().view(np.uint64), wk)


# ---------------------------------------------------------------------- #
# gather_files

GUARD = 0xA5


def _gather_case(dev, rng, rows, dtypes, n_idx, missing):
    """Columns of `dtypes` over files of `rows` rows; `missing[c]` lists the
    files column c has no buffer for (ones). Outputs lie between guard
    bytes in one buffer."""
    from lakesoul_amd.ops import hip

    total = sum(rows)
    idx = rng.integers(0, total, n_idx) if total else np.zeros(0, np.int64)
    cols_np, cols_dev = [], []
    for c, dt in enumerate(dtypes):
        parts = [rng.integers(0, 200, r).astype(dt) for r in rows]
        full = [np.ones(r, dtype=dt) if f in missing[c] else p
                for f, (p, r) in enumerate(zip(parts, rows))]
        cols_np.append(np.concatenate(full) if full else np.zeros(0, dt))
        cols_dev.append([None if f in missing[c] else torch.from_numpy(p).to(dev)
                         for f, p in enumerate(parts)])
    # one guarded buffer: 64 guard bytes, then each output followed by 64
    sizes = [len(idx) * np.dtype(dt).itemsize for dt in dtypes]
    buf = torch.full((64 + sum(s + 64 for s in sizes),), GUARD, dtype=torch.uint8,
                     device=dev)
    outs, pos, spans = [], 64, []
    for dt, s in zip(dtypes, sizes):
        outs.append(buf.narrow(0, pos, s).view(getattr(torch, np.dtype(dt).name)))
        spans.append((pos, pos + s))
        pos += s + 64
    res = hip().gather_files(cols_dev, rows, torch.from_numpy(idx).to(dev), outs)
    host = buf.cpu().numpy()
    for c, (lo, hi) in enumerate(spans):
        got = host[lo:hi].view(dtypes[c])
        np.testing.assert_array_equal(got, cols_np[c][idx])
        np.testing.assert_array_equal(res[c].cpu().numpy(), got)
        host[lo:hi] = GUARD
    assert (host == GUARD).all(), "a byte outside the outputs was written"
    # and with outputs allocated by the binding
    res = hip().gather_files(cols_dev, rows, torch.from_numpy(idx).to(dev))
    for c in range(len(dtypes)):
        np.testing.assert_array_equal(res[c].cpu().numpy(), cols_np[c][idx])


def test_gather_files_esizes(dev):
    """Element sizes 1, 2, 4, 8 over 11 files, one of them empty; a
    validity-like column present in some files only."""
    rng = np.random.default_rng(21)
    rows = [3000, 600, 0, 600, 1, 600, 600, 2049, 600, 600, 7]
    dtypes = [np.uint8, np.int16, np.int32, np.int64, np.uint8]
    missing = [(), (), (), (), (0, 3, 10)]
    _gather_case(dev, rng, rows, dtypes, 5000, missing)


def test_gather_files_tables(dev):
    """37 files (three launches of 16, 16 and 5) with empty files first,
    last and at a table edge, and 19 columns (two column tables)."""
    rng = np.random.default_rng(22)
    rows = [0] + [int(x) for x in rng.integers(1, 90, 35)] + [0]
    rows[15] = rows[16] = 0
    dtypes = [np.uint8, np.int16, np.int32, np.int64] * 4 + [np.uint8] * 3
    missing = [()] * 16 + [(1, 2, 17, 35), tuple(range(16)), (36,)]
    _gather_case(dev, rng, rows, dtypes, 3000, missing)


def test_gather_files_small(dev):
    """One file; no rows taken; a file of one row."""
    rng = np.random.default_rng(23)
    _gather_case(dev, rng, [1], [np.int64, np.uint8], 10, [(), ()])
    _gather_case(dev, rng, [5, 9], [np.int32], 0, [()])
