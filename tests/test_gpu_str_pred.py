"""The string-predicate kernel (csrc/hip/str_pred.hip) against the
plain-Python models of str_pred_cases.py: every case through both forced
shapes (a thread per row, a wave per row), both offset dtypes, slices, nulls,
`out=` between guards; then Cmp / Like on a CUDA batch without a host sync,
and whole scans with each kind of filter."""

import numpy as np
import pytest
import torch
from str_pred_cases import (CMP_OPS, LIKE_BIN_PATTERNS, LIKE_BIN_VALUES,
                            LIKE_PATTERNS, LIKE_STRINGS, LITERAL_LENGTHS, OP_CODE,
                            ROW_COUNTS, cmp_values, column, in_sets, in_values,
                            literal_of, long_cmp_cases, long_like_cases,
                            model_cmp, model_in, model_like, phased)

pytestmark = pytest.mark.gpu

SHAPES = ["rows", "wave"]
LAYOUTS = [(torch.int32, 0), (torch.int64, 0), (torch.int32, 3), (torch.int64, 5)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests require an MI355X"
    return torch.device("cuda:0")


def _cpp():
    from lakesoul_amd.ops import cpp

    return cpp()


def _hip():
    from lakesoul_amd.ops import hip

    return hip()


class DeviceColumn:
    """One column on the device, reused for every predicate over it."""

    def __init__(self, dev, rows, offs_dtype=torch.int32, base_rows=0, null_every=0):
        offs, by, val, self.seen = column(rows, offs_dtype, base_rows, null_every)
        if base_rows:
            assert int(offs[0]) != 0
        self.dev = dev
        self.offs, self.by = offs.to(dev), by.to(dev)
        self.val = None if val is None else val.to(dev)

    def mask(self, op, operand, shape, **kw):
        ob, om = (t.to(self.dev) for t in operand)
        m = _hip().str_pred_mask(self.offs, self.by, self.val, OP_CODE[op], ob, om,
                                 shape=shape, **kw)
        assert m.dtype == torch.bool and m.numel() == len(self.seen)
        return m.cpu().tolist()


# ---------------------------------------------------------------------- #
# comparisons


@pytest.mark.parametrize("offs_dtype,base_rows", LAYOUTS)
@pytest.mark.parametrize("llen", LITERAL_LENGTHS)
def test_compare(dev, llen, offs_dtype, base_rows):
    """Every value length at every byte phase against one literal: equal,
    prefix either way, first / last byte different, the edge bytes; all six
    ordering ops; nulls false for each."""
    lit = literal_of(llen)
    col = DeviceColumn(dev, phased(cmp_values(lit)), offs_dtype, base_rows, null_every=5)
    operand = _cpp().str_pred_compile_literal(lit)
    for op in CMP_OPS:
        want = model_cmp(col.seen, op, lit)
        for shape in SHAPES:
            assert col.mask(op, operand, shape) == want, (op, shape)


def test_compare_long_literal(dev):
    """A 1100-byte literal: differences at the edges of the wave compare's
    512-byte steps, at every phase."""
    lit, vals = long_cmp_cases()
    col = DeviceColumn(dev, phased(vals))
    operand = _cpp().str_pred_compile_literal(lit)
    for op in CMP_OPS:
        want = model_cmp(col.seen, op, lit)
        for shape in SHAPES:
            assert col.mask(op, operand, shape) == want, (op, shape)


@pytest.mark.parametrize("nrows", ROW_COUNTS)
def test_row_counts(dev, nrows):
    vals = [b"abc", b"abd", b"ab", b"", b"abcd", b"b", b"\xff"]
    rows = [vals[(i * 5 + i // 7) % len(vals)] for i in range(nrows)]
    col = DeviceColumn(dev, rows, null_every=6 if nrows > 1 else 0)
    operand = _cpp().str_pred_compile_literal(b"abc")
    for op in CMP_OPS:
        for shape in SHAPES:
            assert col.mask(op, operand, shape) == model_cmp(col.seen, op, b"abc"), (op, shape)


def test_more_rows_than_the_grid(dev):
    """256 x 2048 + 1 short rows: the grid-stride loop goes round, in the
    rows shape twice and in the wave shape 65 times."""
    n = 256 * 2048 + 1
    words = np.array([b"abc", b"abd", b"ab", b"", b"abcd", b"b", b"zz"], dtype=object)
    lens = np.array([len(w) for w in words])
    pick = (np.arange(n) * 5 + np.arange(n) // 7) % len(words)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens[pick], out=offs[1:])
    blob = np.frombuffer(b"".join(words[pick]), dtype=np.uint8).copy()
    validity = (np.arange(n) % 11 != 0).astype(np.uint8)
    o = torch.from_numpy(offs).to(torch.int32).to(dev)
    b, v = torch.from_numpy(blob).to(dev), torch.from_numpy(validity).to(dev)
    for op, lit, fn in (("eq", b"abc", lambda p: p == 0), ("gt", b"abc", lambda p: np.isin(p, [1, 4, 5, 6]))):
        ob, om = (t.to(dev) for t in _cpp().str_pred_compile_literal(lit))
        want = torch.from_numpy(fn(pick) & (validity != 0))
        for shape in SHAPES:
            got = _hip().str_pred_mask(o, b, v, OP_CODE[op], ob, om, shape=shape).cpu()
            assert torch.equal(got, want), (op, shape)
    ob, om = (t.to(dev) for t in _cpp().str_pred_compile_like(b"%b_", ord("\\"), True))
    want = torch.from_numpy(np.isin(pick, [0, 1]) & (validity != 0))
    for shape in SHAPES:
        got = _hip().str_pred_mask(o, b, v, OP_CODE["like"], ob, om, shape=shape).cpu()
        assert torch.equal(got, want), shape


def test_out_between_guards(dev):
    rows = [b"abc", b"x", b"abc", None, b"abcd"] * 13
    col = DeviceColumn(dev, rows)
    operand = _cpp().str_pred_compile_literal(b"abc")
    want = model_cmp(col.seen, "eq", b"abc")
    n = len(rows)
    for shape in SHAPES:
        buf = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device=dev)
        out = buf[7:7 + n].view(torch.bool)
        assert out.data_ptr() % 2 == 1
        got = col.mask("eq", operand, shape, out=out)
        assert got == want and out.data_ptr() == buf.data_ptr() + 7
        host = buf.cpu()
        assert host[7:7 + n].tolist() == [int(x) for x in want]      # 0 / 1 only
        assert set(host[:7].tolist()) == {0xA5} and set(host[7 + n:].tolist()) == {0xA5}
    with pytest.raises(RuntimeError):
        col.mask("eq", operand, "rows", out=torch.empty(n + 1, dtype=torch.bool, device=dev))
    with pytest.raises(RuntimeError):
        col.mask("eq", operand, "diagonal")


# ---------------------------------------------------------------------- #
# IN


@pytest.mark.parametrize("offs_dtype,base_rows", LAYOUTS[:3])
@pytest.mark.parametrize("name", list(in_sets()))
def test_in(dev, name, offs_dtype, base_rows):
    """Set sizes 0, 1, 2 and 7, duplicates, the empty string as a member,
    and one set past the LDS budget, read from global memory."""
    lits = in_sets()[name]
    ob, om = _cpp().str_pred_compile_set(lits)
    staged = ob.numel() + 4 * om.numel() + 16 <= _hip().str_pred_lds_budget()
    assert staged == (name != "big")
    col = DeviceColumn(dev, phased(in_values(lits)) if name != "big" else in_values(lits),
                       offs_dtype, base_rows, null_every=4)
    want = model_in(col.seen, lits)
    assert any(want) == bool(lits)
    for shape in SHAPES:
        assert col.mask("in", (ob, om), shape) == want, shape


# ---------------------------------------------------------------------- #
# LIKE


@pytest.mark.parametrize("offs_dtype,base_rows", LAYOUTS)
def test_like(dev, offs_dtype, base_rows):
    col = DeviceColumn(dev, [s.encode() for s in LIKE_STRINGS], offs_dtype, base_rows,
                       null_every=7)
    for pat in LIKE_PATTERNS:
        operand = _cpp().str_pred_compile_like(pat.encode(), ord("\\"), True)
        for op, neg in (("like", False), ("notlike", True)):
            want = model_like(col.seen, pat, neg)
            for shape in SHAPES:
                assert col.mask(op, operand, shape) == want, (pat, op, shape)


def test_like_binary(dev):
    col = DeviceColumn(dev, LIKE_BIN_VALUES)
    for pat in LIKE_BIN_PATTERNS:
        operand = _cpp().str_pred_compile_like(pat, ord("\\"), False)
        for op, neg in (("like", False), ("notlike", True)):
            want = model_like(col.seen, pat, neg, binary=True)
            for shape in SHAPES:
                assert col.mask(op, operand, shape) == want, (pat, op, shape)


def test_like_fixed_points(dev):
    def like(pat, val, utf8=True):
        operand = _cpp().str_pred_compile_like(pat.encode(), ord("\\"), utf8)
        col = DeviceColumn(dev, [val.encode()])
        got = {col.mask("like", operand, shape)[0] for shape in SHAPES}
        assert len(got) == 1
        return got.pop()

    assert not like("a%a", "a") and like("a%a", "aa")
    assert like("%ab%ab%", "abab") and like("%ab%ab%", "abab ") and not like("%ab%ab%", "aba")
    assert like("_", "é") and like("_", "€") and like("_", "😀")
    assert not like("_", "é", utf8=False) and like("__", "é", utf8=False)
    assert like("100\\%", "100%") and not like("100\\%", "1000")
    assert like("a\\_c", "a_c") and not like("a\\_c", "abc") and like("a\\\\c", "a\\c")


def test_like_long_values(dev):
    """1 KB and 5000-byte values: the only match at the very end, matches
    that start at 63, 64, 65, a middle segment longer than 64 bytes."""
    for name, pat, vals in long_like_cases():
        # row 0 is a NULL of its own, so that no case loses its one match
        col = DeviceColumn(dev, [b"-"] + [v.encode() for v in vals], null_every=30)
        operand = _cpp().str_pred_compile_like(pat.encode(), ord("\\"), True)
        want = model_like(col.seen, pat)
        assert any(want) and not all(want), name
        for shape in SHAPES:
            assert col.mask("like", operand, shape) == want, (name, shape)


def test_host_and_device_agree_on_broken_utf8(dev):
    rows = [b"\xc3", b"a\xc3", b"\xa9\xa9", b"a\xe2\x82", b"\xf0\x9fx", b"\x80a\x80",
            b"\xff\xff", b"ab\xc3", b"\xc3\xc3\xa9\xa9", b""]
    col = DeviceColumn(dev, rows)
    offs, by, val, _ = column(rows)
    for pat in (b"_", b"__", b"%_", b"_%", b"%\xa9", b"a_", b"%_\x80", b"\xc3_", b"%_%_%"):
        ob, om = _cpp().str_pred_compile_like(pat, ord("\\"), True)
        host = _cpp().str_pred_mask(offs, by, val, OP_CODE["like"], ob, om).tolist()
        for shape in SHAPES:
            assert col.mask("like", (ob, om), shape) == host, (pat, shape)


# ---------------------------------------------------------------------- #
# Cmp / Like on a CUDA batch

TABLE_S = ["apple", "apricot", None, "banana", "a", "", "grape_1", "50%", "açaí",
           "a%", None, "Apple", "pineapple", "ap", "x" * 700 + "apple"]


def _batches(dev, strings=TABLE_S):
    from lakesoul_amd.io.batch import Batch, Column
    from lakesoul_amd.io.schema import Field, Schema

    schema = Schema([Field("id", "int64", False), Field("s", "string"),
                     Field("b", "binary")])
    out = []
    for d in (torch.device("cpu"), dev):
        cols = {"id": Column("int64", data=torch.arange(len(strings)).to(d))}
        for name, dt in (("s", "string"), ("b", "binary")):
            offs, by, val, _ = column([None if s is None else s.encode() for s in strings])
            cols[name] = Column(dt, offsets=offs.to(d), bytes_=by.to(d),
                                validity=None if val is None else val.to(d))
        out.append(Batch(schema, cols))
    return out


def _exprs():
    from lakesoul_amd.io.filters import And, Cmp, Like, Not, Or

    return [Cmp("s", op, v) for op in CMP_OPS for v in ("apple", "", "açaí")] + [
        Cmp("s", "in", ["apple", "a", "nope", ""]), Cmp("s", "in", []),
        Cmp("b", "in", [b"ap", b"Apple"]), Cmp("b", "lt", b"b"),
        Like("s", "a%"), Like("s", "a%", negate=True), Like("s", "%pp%"),
        Like("s", "_ç%"), Like("b", b"_\xc3%"), Like("s", "50!%", escape="!"),
        Like("s", "%apple"),
        And(Like("s", "a%"), Not(Cmp("s", "eq", "apple"))),
        Or(Like("s", "%e"), Cmp("id", "lt", 2)),
    ]


def test_evaluate_equals_cpu_and_does_not_sync(dev):
    """Masks on a CUDA batch equal the CPU evaluation of the same batch, and
    evaluating (fresh expressions: operand compile and upload included) makes
    no host sync and no device-to-host copy."""
    cpu_batch, gpu_batch = _batches(dev)
    want = [e.evaluate(cpu_batch) for e in _exprs()]
    fresh = _exprs()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [e.evaluate(gpu_batch) for e in fresh]
        again = [e.evaluate(gpu_batch) for e in fresh]      # cached operands
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for e, w, g, a in zip(fresh, want, got, again):
        assert g.is_cuda and g.dtype == torch.bool
        assert torch.equal(g.cpu(), w), e
        assert torch.equal(a.cpu(), w), e
    # the mode does trip on what the old path did
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            gpu_batch.columns["s"].offsets.cpu()
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_shape_picked_from_mean_length(dev):
    """No shape forced: the thresholds between the shapes (the crossovers
    measured in profiles/r07_gpu_str_pred.md), and long values through
    Cmp / Like, where the wave shape is the one picked."""
    from lakesoul_amd.io.batch import Batch, Column
    from lakesoul_amd.io.filters import Cmp, Like
    from lakesoul_amd.io.schema import Field, Schema

    pick = _hip().str_pred_pick_shape
    for op in CMP_OPS + ["in"]:
        assert pick(OP_CODE[op], 1000, 1000 * 1023) == "rows"
        assert pick(OP_CODE[op], 1000, 1000 * 1024) == "wave"
    for op in ("like", "notlike"):
        assert pick(OP_CODE[op], 1000, 1000 * 95) == "rows"
        assert pick(OP_CODE[op], 1000, 1000 * 96) == "wave"
    assert pick(0, 0, 0) == "rows"
    lit, vals = long_cmp_cases()
    cases = [(vals + [lit * 3] * 8, [Cmp("s", op, lit) for op in CMP_OPS] + [Cmp("s", "in", vals[:7])],
              "binary")]
    for name, pat, strs in long_like_cases():
        cases.append(([v.encode() for v in strs], [Like("s", pat), Like("s", pat, negate=True)],
                      "string"))
    for rows, exprs, dtype in cases:
        offs, by, val, seen = column(rows, null_every=len(rows) - 1)
        assert pick(7, len(rows), by.numel()) == "wave"
        schema = Schema([Field("s", dtype)])
        cpu = Batch(schema, {"s": Column(dtype, offsets=offs, bytes_=by, validity=val)})
        gpu = Batch(schema, {"s": Column(dtype, offsets=offs.to(dev), bytes_=by.to(dev),
                                         validity=val.to(dev))})
        for e in exprs:
            if isinstance(e, Like):
                want = model_like(seen, e.pattern, e.negate)
            elif e.op == "in":
                want = model_in(seen, e.value)
            else:
                want = model_cmp(seen, e.op, e.value)
            assert e.evaluate(gpu).cpu().tolist() == want, e
            assert e.evaluate(cpu).tolist() == want, e


# ---------------------------------------------------------------------- #
# whole scans


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    from lakesoul_amd.io.schema import Field, Schema
    from lakesoul_amd.meta.client import MetaClient
    from lakesoul_amd.meta.store import SqliteMetaStore
    from lakesoul_amd.tables.catalog import LakeSoulCatalog

    td = tmp_path_factory.mktemp("str_pred_scan")
    catalog = LakeSoulCatalog(MetaClient(SqliteMetaStore(str(td / "meta.db"))),
                              warehouse=str(td / "wh"))
    t = catalog.create_table("likes", Schema([Field("id", "int64", False),
                                              Field("s", "string")]),
                             primary_keys=["id"], hash_bucket_num=2)
    n = 600
    words = ["apple", "apricot", None, "banana", "a", "", "grape_1", "50%", "açaí", "a%"]
    s = [None if words[i % 10] is None else words[i % 10] + ("" if i % 3 else str(i))
         for i in range(n)]
    t.upsert({"id": np.arange(n, dtype=np.int64), "s": list(s)}, device="cuda")
    for i in range(0, n, 7):
        s[i] = None if i % 2 else "avocado%d" % i
    t.upsert({"id": np.arange(0, n, 7, dtype=np.int64), "s": [s[i] for i in range(0, n, 7)]},
             device="cuda")
    return catalog, t, s


def _scan_ids(t, filters, device):
    df = t.scan(filters=filters, device=device).to_arrow().to_pandas()
    return sorted(df["id"].tolist())


def test_filtered_scans(dev, table):
    from lakesoul_amd.io.filters import Cmp, Like
    from lakesoul_amd.io.substrait import encode_substrait_filter

    catalog, t, s = table
    enc = [None if x is None else x.encode() for x in s]

    def ids(mask):
        return [i for i, m in enumerate(mask) if m]

    cases = [
        ([("s", "=", "apple")], ids(model_cmp(enc, "eq", b"apple"))),
        ([("s", ">=", "b")], ids(model_cmp(enc, "gteq", b"b"))),
        ([("s", "in", ["apple", "avocado0", "", "a%"])],
         ids(model_in(enc, [b"apple", b"avocado0", b"", b"a%"]))),
        ([("s", "like", "a%1_")], ids(model_like(enc, "a%1_"))),
        ([("s", "not like", "a%")], ids(model_like(enc, "a%", negate=True))),
        ([("s", "contains", "%")], ids(model_like(enc, "%\\%%"))),
        ("like(s,'_ç%')", ids(model_like(enc, "_ç%"))),
        ("and(startswith(s,'a'),noteq(s,'a'))",
         ids([a and b for a, b in zip(model_like(enc, "a%"), model_cmp(enc, "noteq", b"a"))])),
        (Like("s", "%o%", negate=True), ids(model_like(enc, "%o%", negate=True))),
        (encode_substrait_filter(Like("s", "avocado%"), t.schema), ids(model_like(enc, "avocado%"))),
        (encode_substrait_filter(Cmp("s", "in", ["banana", "a"]), t.schema),
         ids(model_in(enc, [b"banana", b"a"]))),
    ]
    for filters, want in cases:
        assert want, filters
        assert _scan_ids(t, filters, "cuda") == want, filters
        assert _scan_ids(t, filters, "cpu") == want, filters


def test_execute_sql_like(dev, table):
    from lakesoul_amd.sql import execute_sql

    catalog, t, s = table
    enc = [None if x is None else x.encode() for x in s]
    for cond, want in (
            ("s like 'a%'", model_like(enc, "a%")),
            ("s not like 'a%'", model_like(enc, "a%", negate=True)),
            ("s like '50!%%' escape '!'", model_like(enc, "50!%%", escape="!")),
            ("s in ('apple', 'a') or s like '%9'",
             [a or b for a, b in zip(model_in(enc, [b"apple", b"a"]), model_like(enc, "%9"))])):
        want_ids = [i for i, m in enumerate(want) if m]
        assert want_ids, cond
        for device in ("cuda", "cpu"):
            df = execute_sql(catalog, f"select id from likes where {cond}", device=device)
            assert sorted(df["id"].tolist()) == want_ids, (cond, device)
