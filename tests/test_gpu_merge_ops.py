"""The GPU merge (merge_gpu.merge_sorted_files_gpu and its kernels) against
merge_cpu.merge_sorted_files and a few lines of numpy: every merge
operator and value dtype, every PK kind with the integer extremes and
byte-string keys, nulls, partial columns, duplicate keys inside a file,
CDC deletes, and inputs long enough for the grid-stride loops to iterate.
tests/test_merge_model.py holds merge_cpu itself to a plain model."""

import math
import zlib

import numpy as np
import pytest
import torch
from merge_model import (JOIN_OPS, PACKED_PK_KINDS, PK_KINDS,
                         STRING_KEY_ALPHABET, SUM_OPS, assert_input_conditions,
                         batch_to_lists, columns_to_lists, compare_exact,
                         compare_to_model, gen_case, model_merge, wrap)

pytestmark = pytest.mark.gpu

SHAPES = [[0], [1], [0, 7], [30, 0, 30], [40, 40, 40, 40, 3]]
# the merge tile is 2048 keys; three streams carry an odd one forward
TILE_SHAPES = [[2047, 2049], [1, 4100, 7]]

_FIXED = ["int8", "int16", "int32", "int64", "float32", "float64"]
OP_DTYPE = (
    [(op, dt) for op in ("UseLast", "UseLastNotNull")
     for dt in _FIXED + ["bool", "string"]]
    + [(op, dt) for op in SUM_OPS for dt in _FIXED + ["decimal(12,2)"]]
    + [(op, "string") for op in JOIN_OPS])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests require an MI355X"
    return torch.device("cuda:0")


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def run_case(dev, case, ops, partial=None):
    """GPU merge == CPU merge on one case, value by value; both within the
    float-sum bound of the model's addends."""
    from lakesoul_amd.io.merge_cpu import merge_sorted_files
    from lakesoul_amd.io.merge_gpu import merge_sorted_files_gpu

    assert_input_conditions(case, ops.get("v", "UseLast"), partial)
    model = model_merge(case.files, case.pk, ops, case.present, case.cdc)
    cpu = columns_to_lists(merge_sorted_files(
        case.np_files(), case.pk, ops, case.cdc, case.present))
    compare_to_model(cpu, model, case.fields, ops, case.pk)
    out = merge_sorted_files_gpu(case.device_batches(dev), case.pk, ops,
                                 case.cdc, case.present)
    gpu = batch_to_lists(out)
    compare_exact(gpu, cpu, case.fields, ops, case.pk)
    compare_to_model(gpu, model, case.fields, ops, case.pk)
    return gpu, model


# ---------------------------------------------------------------------- #
# merge_sorted_files_gpu vs merge_cpu


@pytest.mark.parametrize("pk_kind", PK_KINDS)
def test_merge_pk_kinds(dev, pk_kind):
    """Every PK kind over every shape: the all-UseLast path (one fused
    gather) with CDC, and the operator path with nulls, a partial column
    and CDC. Packed integer PKs also cross the merge tile."""
    rng = np.random.default_rng(_seed("pk", pk_kind))
    shapes = [(s, 24, "odd") for s in SHAPES]
    if pk_kind in PACKED_PK_KINDS:
        # [1, 4100, 7] keeps its column in every file: without the middle
        # file 8 rows would be left to take part
        shapes += [(TILE_SHAPES[0], 300, "odd"), (TILE_SHAPES[1], 300, None)]
    rows = 0
    for sizes, ndomain, partial in shapes:
        case = gen_case(rng, pk_kind, "int64", sizes, 0.3, None, cdc=True,
                        ndomain=ndomain)
        gpu, _ = run_case(dev, case, {})
        rows += len(gpu["v"])
        case = gen_case(rng, pk_kind, "int32", sizes, 0.3, partial, cdc=True,
                        ndomain=ndomain)
        run_case(dev, case, {"v": "SumLast"}, partial)
    assert rows > 0


@pytest.mark.parametrize("op,vdtype", OP_DTYPE,
                         ids=[f"{o}-{d}" for o, d in OP_DTYPE])
def test_merge_operator_dtype(dev, op, vdtype):
    """One operator on one value dtype: with and without nulls; all files
    with the column, odd-numbered files without it, and groups none of
    whose files has it; a packed, a composite and a string PK."""
    rng = np.random.default_rng(_seed("op", op, vdtype))
    kinds = ["int64", "int32+int32", "int64+string"]
    i = 0
    for null_p in (0.0, 0.3):
        for partial in (None, "odd", "group"):
            case = gen_case(rng, kinds[i % 3], vdtype, [40, 40, 40, 40, 3],
                            null_p, partial, cdc=i % 2 == 1)
            _, model = run_case(dev, case, {"v": op}, partial)
            if partial == "group":  # a group with no participant at all
                assert any(m is None or m == [] or m == b""
                           for m in model["v"])
            i += 1
    case = gen_case(rng, "string", vdtype, [30, 0, 30], 0.3, "odd")
    run_case(dev, case, {"v": op}, "odd")


@pytest.mark.parametrize("op,vdtype", [
    ("UseLast", "int64"), ("UseLastNotNull", "float32"), ("SumAll", "int16"),
    ("SumLast", "float64"), ("JoinedAllByComma", "string"),
    ("JoinedLastBySemicolon", "string")])
def test_merge_all_null_column(dev, op, vdtype):
    rng = np.random.default_rng(_seed("allnull", op))
    case = gen_case(rng, "int32+int32", vdtype, [30, 0, 30], 1.0, None)
    gpu, _ = run_case(dev, case, {"v": op})
    assert gpu["v"] and all(v is None for v in gpu["v"])


# ---------------------------------------------------------------------- #
# through the table layer


def _mk_catalog(tmp_path):
    from lakesoul_amd.meta.client import MetaClient
    from lakesoul_amd.meta.store import SqliteMetaStore
    from lakesoul_amd.tables.catalog import LakeSoulCatalog

    store = SqliteMetaStore(str(tmp_path / "meta.db"))
    return LakeSoulCatalog(MetaClient(store), warehouse=str(tmp_path / "wh"))


def _count_calls(monkeypatch, owner, name):
    calls = []
    real = getattr(owner, name)

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(owner, name, spy)
    return calls


@pytest.mark.parametrize("id_dtype", ["int64", "int32"])
def test_scan_uselast_extreme_ids(dev, tmp_path, monkeypatch, id_dtype):
    """The one-call unit path (scan_unit_uselast: pack, merge, keep_last,
    gather) on ids with negatives and the type's ends; int32 ids are
    widened before the pack."""
    import pandas as pd

    import lakesoul_amd._hip as hipmod
    from lakesoul_amd.io.schema import Field, Schema

    npdt = np.dtype(id_dtype)
    info = np.iinfo(npdt)
    t = _mk_catalog(tmp_path).create_table(
        "ext_" + id_dtype,
        Schema([Field("id", id_dtype, False), Field("v", "float64"),
                Field("s", "string")]),
        primary_keys=["id"], hash_bucket_num=2)
    rng = np.random.default_rng(_seed("table", id_dtype))
    ends = np.array([info.min, info.min + 1, -1, 0, 1, info.max - 1, info.max],
                    dtype=npdt)
    domain = np.unique(np.concatenate(
        [ends, rng.integers(info.min, info.max, 500, dtype=npdt),
         rng.integers(-300, 300, 200).astype(npdt)]))
    expect = {}
    for it, n in enumerate((400, 300, 300)):
        ids = np.unique(np.concatenate(
            [ends[it::2], rng.choice(domain, n, replace=False)]))
        v = rng.normal(size=len(ids))
        t.upsert({"id": ids, "v": v, "s": [f"u{it}_{i}" for i in ids]})
        expect.update({int(i): (x, f"u{it}_{i}") for i, x in zip(ids, v)})
    calls = _count_calls(monkeypatch, hipmod, "scan_unit_uselast")
    gpu = t.scan(device="cuda").to_arrow().to_pandas()
    assert calls, "scan did not take the one-call unit path"
    cpu = t.scan(device="cpu").to_arrow().to_pandas()
    cpu = cpu.sort_values("id").reset_index(drop=True)
    gpu = gpu.sort_values("id").reset_index(drop=True)
    pd.testing.assert_frame_equal(cpu, gpu)
    assert gpu["id"].tolist() == sorted(expect)
    assert gpu["v"].tolist() == [expect[i][0] for i in sorted(expect)]
    assert gpu["s"].tolist() == [expect[i][1] for i in sorted(expect)]
    assert gpu["id"].iloc[0] == info.min and gpu["id"].iloc[-1] == info.max


def test_scan_sumlast_joinedlast_repeated_ids(dev, tmp_path, monkeypatch):
    """merge_op.* = SumLast / JoinedLastByComma through the generic scan
    path, with ids repeated inside one upsert batch: only the last row per
    file and id takes part."""
    import lakesoul_amd.io.reader_gpu as rgpu
    from lakesoul_amd.io.schema import Field, Schema

    t = _mk_catalog(tmp_path).create_table(
        "sumlast",
        Schema([Field("id", "int64", False), Field("x", "float64"),
                Field("tags", "string")]),
        primary_keys=["id"], hash_bucket_num=2,
        properties={"merge_op.x": "SumLast",
                    "merge_op.tags": "JoinedLastByComma"})
    rng = np.random.default_rng(_seed("table", "sumlast"))
    files = []
    for it, n in enumerate((300, 400, 200)):
        # the second batch draws 400 ids from 150: most ids repeat
        ids = rng.integers(-100, 200 if it != 1 else 50, n).astype(np.int64)
        x = np.array([float(np.float32(rng.standard_normal() * 10.0 ** k))
                      for k in rng.integers(-3, 4, n)])
        tags = [f"t{it}.{j}" for j in range(n)]
        t.upsert({"id": ids, "x": x, "tags": tags})
        order = np.argsort(ids, kind="stable")
        files.append({"id": ids[order].tolist(), "x": x[order].tolist(),
                      "tags": [tags[j].encode() for j in order]})
    assert len(set(files[1]["id"])) < len(files[1]["id"])
    ops = {"x": "SumLast", "tags": "JoinedLastByComma"}
    fields = [("id", "int64"), ("x", "float64"), ("tags", "string")]
    model = model_merge(files, ["id"], ops)
    calls = _count_calls(monkeypatch, rgpu, "merge_sorted_files_gpu")
    results = {}
    for device in ("cuda", "cpu"):
        tbl = t.scan(device=device).to_arrow().sort_by("id")
        results[device] = {
            "id": tbl.column("id").to_pylist(),
            "x": tbl.column("x").to_pylist(),
            "tags": [None if s is None else s.encode()
                     for s in tbl.column("tags").to_pylist()]}
        compare_to_model(results[device], model, fields, ops, ["id"])
    assert calls, "scan did not reach merge_sorted_files_gpu"
    compare_exact(results["cuda"], results["cpu"], fields, ops, ["id"])
    assert any(b"," in s for s in results["cuda"]["tags"])
    # SumLast is not SumAll here: some id has more rows than addends
    all_rows = model_merge(files, ["id"], {"x": "SumAll"})["x"]
    assert any(len(a) < len(b) for a, b in zip(model["x"], all_rows))
    assert any(len(a) >= 2 for a in model["x"])


# ---------------------------------------------------------------------- #
# kernels, one binding at a time

_I64_ENDS = [-2 ** 63, -2 ** 63 + 1, -1, 0, 1, 2 ** 31, 2 ** 63 - 2, 2 ** 63 - 1]
_I32_ENDS = [-2 ** 31, -2 ** 31 + 1, -1, 0, 1, 2 ** 31 - 2, 2 ** 31 - 1]
_FLIP = np.uint64(1 << 63)


def _to(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def test_pack_key_i64(dev):
    from lakesoul_amd.ops import hip

    rng = np.random.default_rng(10)
    x = np.concatenate([np.array(_I64_ENDS, dtype=np.int64),
                        rng.integers(-2 ** 63, 2 ** 63 - 1, 500)])
    rng.shuffle(x)
    got = _u64(hip().pack_key_i64(_to(dev, x)))
    np.testing.assert_array_equal(got, x.view(np.uint64) ^ _FLIP)
    np.testing.assert_array_equal(x[np.argsort(got, kind="stable")],
                                  np.sort(x, kind="stable"))


def test_pack_key_2xi32(dev):
    from lakesoul_amd.ops import hip

    rng = np.random.default_rng(11)
    ends = np.array(_I32_ENDS, dtype=np.int32)
    # every pair of ends: equal hi with lo on both sides of the sign
    hi = np.concatenate([np.repeat(ends, len(ends)),
                         rng.integers(-2 ** 31, 2 ** 31 - 1, 300, dtype=np.int32)])
    lo = np.concatenate([np.tile(ends, len(ends)),
                         rng.integers(-2 ** 31, 2 ** 31 - 1, 300, dtype=np.int32)])
    perm = rng.permutation(len(hi))
    hi, lo = hi[perm], lo[perm]
    got = _u64(hip().pack_key_2xi32(_to(dev, hi), _to(dev, lo)))
    h = hi.view(np.uint32).astype(np.uint64) ^ np.uint64(1 << 31)
    l = lo.view(np.uint32).astype(np.uint64) ^ np.uint64(1 << 31)
    np.testing.assert_array_equal(got, (h << np.uint64(32)) | l)
    order = np.argsort(got, kind="stable")
    want = np.lexsort((lo, hi))
    np.testing.assert_array_equal(hi[order], hi[want])
    np.testing.assert_array_equal(lo[order], lo[want])


def test_group_start_mask(dev):
    from lakesoul_amd.ops import hip

    def check(k):
        k = np.asarray(k, dtype=np.uint64)
        got = hip().group_start_mask(_to(dev, k.view(np.int64))).cpu().numpy()
        np.testing.assert_array_equal(
            got.astype(bool), np.r_[True, k[1:] != k[:-1]])

    check([5])
    check([0, 0, 1, 1, 1 << 63, 1 << 63, (1 << 63) | 1, (1 << 63) | 1,
           (1 << 64) - 1])
    check([0, 1 << 63])   # differ in bit 63 only
    check([6, 7, 7])      # differ in bit 0 only
    check(np.sort(np.random.default_rng(12).integers(0, 300, 3000)))


def _chunk_key(s, ci):
    word = int.from_bytes(s[8 * ci:8 * ci + 8].ljust(8, b"\x00"), "big")
    return wrap(word ^ (1 << 63), 64)


def test_str_chunk_keys(dev):
    """8-byte big-endian chunk keys, zero-padded, sign-flipped: chunks 0-2
    of the key alphabet and chunk 3, past the end of every string; the
    numpy mirror in _string_sort_tensors gives the same words."""
    from lakesoul_amd.io.batch import Column
    from lakesoul_amd.io.merge_gpu import _string_sort_tensors
    from lakesoul_amd.ops import hip

    rows = STRING_KEY_ALPHABET + STRING_KEY_ALPHABET[::-1]
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(r) for r in rows])
    by = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
    assert max(len(r) for r in rows) == 17
    for ci in range(4):
        got = hip().str_chunk_keys(_to(dev, offs), _to(dev, by), ci)
        assert got.cpu().tolist() == [_chunk_key(r, ci) for r in rows], ci
    col = Column("string", offsets=torch.from_numpy(offs),
                 bytes_=torch.from_numpy(by))
    mirror = _string_sort_tensors([col], torch.device("cpu"))
    assert len(mirror) == 4  # three chunks, then the lengths
    for ci in range(3):
        assert mirror[ci].tolist() == [_chunk_key(r, ci) for r in rows]
    assert mirror[3].tolist() == [len(r) for r in rows]


def _segments(rng, n, ngroups):
    """Sorted group ids covering 0..ngroups-1, uneven group sizes."""
    cuts = np.sort(rng.choice(np.arange(1, n), ngroups - 1, replace=False))
    grp = np.zeros(n, dtype=np.int64)
    grp[cuts] = 1
    return np.cumsum(grp)


_MASKS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize("dtype", ["float32", "float64", "int32", "int64"])
def test_segmented_sum(dev, dtype):
    from lakesoul_amd.ops import hip

    rng = np.random.default_rng(_seed("segsum", dtype))
    n, ngroups = 5000, 300
    grp = _segments(rng, n, ngroups)
    if dtype.startswith("int"):
        info = np.iinfo(dtype)
        vals = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
        vals[:40] = np.tile([info.min, info.max], 20)
    else:
        vals = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
                ).astype(np.float32).astype(dtype)
    empty = torch.empty(0, dtype=torch.uint8, device=dev)
    for with_contrib, with_valid in _MASKS:
        contrib = (rng.random(n) < 0.6).astype(np.uint8)
        valid = (rng.random(n) < 0.97).astype(np.uint8)
        contrib[grp == 7] = 0          # a group with no contributor
        sums, has_null = hip().segmented_sum(
            _to(dev, vals), _to(dev, grp),
            _to(dev, contrib) if with_contrib else empty,
            _to(dev, valid) if with_valid else empty, ngroups)
        sums, has_null = sums.cpu().numpy(), has_null.cpu().numpy()
        assert sums.dtype == np.dtype(dtype)
        addends = [[] for _ in range(ngroups)]
        null = [False] * ngroups
        for i in range(n):
            if with_contrib and not contrib[i]:
                continue
            if with_valid and not valid[i]:
                null[grp[i]] = True
                continue
            addends[grp[i]].append(vals[i].item())
        assert [bool(x) for x in has_null] == null
        if with_contrib:
            assert addends[7] == [] and sums[7] == 0
        for g, a in enumerate(addends):
            if dtype.startswith("int"):
                assert sums[g].item() == wrap(sum(a), np.iinfo(dtype).bits), g
            else:
                bound = len(a) * float(np.finfo(dtype).eps) * math.fsum(
                    abs(x) for x in a)
                assert abs(sums[g].item() - math.fsum(a)) <= bound, g


def test_segmented_last(dev):
    from lakesoul_amd.ops import hip

    rng = np.random.default_rng(13)
    n, ngroups = 5000, 300
    grp = _segments(rng, n, ngroups)
    empty = torch.empty(0, dtype=torch.uint8, device=dev)
    for with_contrib, with_valid in _MASKS:
        contrib = (rng.random(n) < 0.5).astype(np.uint8)
        valid = (rng.random(n) < 0.5).astype(np.uint8)
        contrib[grp == 7] = 0
        valid[grp == 9] = 0
        got = hip().segmented_last(
            _to(dev, grp), _to(dev, contrib) if with_contrib else empty,
            _to(dev, valid) if with_valid else empty, ngroups, n)
        want = [-1] * ngroups
        for i in range(n):
            if with_contrib and not contrib[i]:
                continue
            if with_valid and not valid[i]:
                continue
            want[grp[i]] = i
        assert got.cpu().tolist() == want
        assert (want[7] == -1) == with_contrib
        assert (want[9] == -1) == with_valid


def test_bytes_ne_mask(dev):
    from lakesoul_amd.ops import hip

    rows = [b"delete", b"", b"delet", b"deletee", b"delett", b"Delete",
            b"xdelet", b"delete", b"e", b"deletedelete", b"", b"delete"]
    offs = np.zeros(len(rows) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(r) for r in rows])
    by = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
    pattern = np.frombuffer(b"delete", dtype=np.uint8).copy()
    got = hip().bytes_ne_mask(_to(dev, offs), _to(dev, by), _to(dev, pattern))
    assert got.cpu().tolist() == [int(r != b"delete") for r in rows]


def test_gather_fixed_multi_two_launches(dev):
    """17 columns in one call (16 per launch), element sizes 1, 2, 4, 8,
    a [rows, 2] int32 column, an index with repeats."""
    from lakesoul_amd.ops import hip

    rng = np.random.default_rng(14)
    rows, n = 1000, 3000
    dtypes = [np.uint8, np.int8, np.int16, np.float16, np.int32, np.float32,
              np.int64, np.float64] * 2
    cols = [rng.integers(-100, 100, rows).astype(dt) for dt in dtypes]
    cols.insert(5, rng.integers(-2 ** 31, 2 ** 31 - 1, (rows, 2), dtype=np.int32))
    assert len(cols) == 17
    idx = rng.integers(0, rows, n)
    idx[:10] = idx[10]
    outs = hip().gather_fixed_multi([_to(dev, c) for c in cols], _to(dev, idx))
    assert len(outs) == 17
    for c, o in zip(cols, outs):
        got = o.cpu().numpy()
        assert got.dtype == c.dtype
        np.testing.assert_array_equal(got, c[idx])


def test_grid_stride_loops(dev):
    """n = 2048 blocks x 256 threads + 257: the elementwise kernels take a
    second trip through their grid-stride loops."""
    from lakesoul_amd.ops import hip
    from lakesoul_amd.utils import murmur3_np

    n = 2048 * 256 + 257
    rng = np.random.default_rng(15)
    empty_u8 = torch.empty(0, dtype=torch.uint8, device=dev)
    empty_i64 = torch.empty(0, dtype=torch.int64, device=dev)
    x = rng.integers(-2 ** 63, 2 ** 63 - 1, n)
    xd = _to(dev, x)

    np.testing.assert_array_equal(_u64(hip().pack_key_i64(xd)),
                                  x.view(np.uint64) ^ _FLIP)

    keys = np.sort(rng.integers(0, n // 3, n)).astype(np.uint64)
    start = hip().group_start_mask(_to(dev, keys.view(np.int64))).cpu().numpy()
    want_start = np.r_[True, keys[1:] != keys[:-1]]
    np.testing.assert_array_equal(start.astype(bool), want_start)

    grp = np.cumsum(want_start) - 1
    ngroups = int(grp[-1]) + 1
    contrib = (rng.random(n) < 0.7).astype(np.uint8)
    valid = (rng.random(n) < 0.999).astype(np.uint8)
    use = contrib.astype(bool) & valid.astype(bool)
    sums, has_null = hip().segmented_sum(
        xd, _to(dev, grp), _to(dev, contrib), _to(dev, valid), ngroups)
    want = np.zeros(ngroups, dtype=np.int64)
    np.add.at(want, grp[use], x[use])
    np.testing.assert_array_equal(sums.cpu().numpy(), want)
    want_null = np.zeros(ngroups, dtype=bool)
    want_null[grp[contrib.astype(bool) & ~valid.astype(bool)]] = True
    np.testing.assert_array_equal(has_null.cpu().numpy().astype(bool), want_null)

    last = hip().segmented_last(_to(dev, grp), _to(dev, contrib),
                                _to(dev, valid), ngroups, n)
    want_last = np.full(ngroups, -1, dtype=np.int64)
    np.maximum.at(want_last, grp[use], np.flatnonzero(use))
    np.testing.assert_array_equal(last.cpu().numpy(), want_last)

    h = hip().hash_fixed_column(xd, empty_u8, empty_i64, True)
    want_h = murmur3_np.hash_column(x, murmur3_np.HASH_SEED)
    np.testing.assert_array_equal(h.cpu().numpy(), want_h.astype(np.int64))
    assert int(want_h.max()) >= 2 ** 31
    b = hip().bucket_ids(h, 1000).cpu().numpy()
    np.testing.assert_array_equal(b, want_h % np.uint32(1000))


def test_merge_pairs_tile_stride(dev):
    """2048 tiles of 2048 keys and 5000 more: blocks of the merge take a
    second tile. Few distinct keys, so ties cross every tile edge."""
    from lakesoul_amd.ops import hip

    total = 2048 * 2048 + 5000
    rng = np.random.default_rng(16)
    na = total * 3 // 5
    streams = [np.sort(rng.integers(0, 200000, m)) for m in (na, total - na)]
    keys, order = hip().merge_sorted_keys([_to(dev, s) for s in streams])
    concat = np.concatenate(streams)
    want = np.argsort(concat, kind="stable")
    np.testing.assert_array_equal(order.cpu().numpy(), want)
    np.testing.assert_array_equal(keys.cpu().numpy(), concat[want])
