"""LZ4 on the host: the block decoder and encoder (csrc/cpp/lz4_dec.h)
against liblz4 (through pyarrow) and the hand-built corpus
(tests/lz4_corpus.py); Hadoop framing (parquet codec 5); LZ4_RAW (codec 7)
parquet files read and written; the C ABI; the sanitizer program."""

import os
import shutil
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from lakesoul_amd.ops import cpp

import lz4_corpus as lc
from test_capi import lib  # noqa: F401  (the ctypes loader fixture)

CODEC = pa.Codec("lz4_raw")


# ---- decoder ---------------------------------------------------------- #

def test_decoder_on_corpus():
    names = set()
    for name, block, orig in lc.entries():
        names.add(name)
        assert cpp().lz4_block_decode_ref(block, len(orig)) == orig, name
        assert lc.liblz4_decode(block, len(orig)) == orig, name
        # the page's size is part of the question
        assert cpp().lz4_block_decode_ref(block, len(orig) + 1) is None, name
        if orig:
            assert cpp().lz4_block_decode_ref(block, len(orig) - 1) is None, name
    assert len(names) == len(lc.entries()) >= 120
    # the extension bytes the corpus is built for
    by_name = {n: b for n, b, _ in lc.entries()}
    assert by_name["lit_15"][20:][:2] == b"\xf2\x00"
    assert by_name["lit_269"][20:][:2] == b"\xf2\xfe"
    assert by_name["lit_270"][20:][:3] == b"\xf2\xff\x00"
    assert by_name["lit_271"][20:][:3] == b"\xf2\xff\x01"
    # real blocks: incompressible shapes are one literal run, the others
    # hold matches
    for n, b, o in lc.entries():
        if n in ("f64_131072", "f32_131072", "i64wide_131072"):
            assert len(b) > len(o) and lc.decode(b[:]) == o
        if n in ("ids_131072", "i32small_131072"):
            assert len(b) < 0.8 * len(o), (n, len(b))


def test_block_that_ends_in_a_match_is_refused():
    blk = lc.seq(b"abcdefgh", 8, 8)  # no closing literals
    assert cpp().lz4_block_decode_ref(blk, 16) is None
    assert cpp().lz4_block_decode_ref(blk + lc.seq(b"12345"), 21) == \
        b"abcdefgh" * 2 + b"12345"
    # offset 0, offset past the output
    assert cpp().lz4_block_decode_ref(
        b"\x40abcd\x00\x00" + lc.seq(b"12345"), 13) is None
    assert cpp().lz4_block_decode_ref(
        lc.seq(b"abcd", 5, 4) + lc.seq(b"12345"), 13) is None
    # extension bytes that run into the end of the block
    assert cpp().lz4_block_decode_ref(b"\xf0" + b"\xff" * 4000, 1 << 20) is None
    assert cpp().lz4_block_decode_ref(b"\x1fx\x01\x00" + b"\xff" * 4000, 1 << 20) is None
    assert cpp().lz4_block_decode_ref(b"", 0) is None


# ---- encoder ---------------------------------------------------------- #

def _round_trip(data: bytes):
    blk = cpp().lz4_compress_ref(data)
    assert cpp().lz4_block_decode_ref(blk, len(data)) == data
    assert lc.liblz4_decode(blk, len(data)) == data
    assert lc.decode(blk) == data
    return blk


def test_encoder_round_trips():
    rng = np.random.default_rng(9)
    for n in range(0, 41):
        for data in (bytes(rng.integers(0, 256, n, dtype=np.uint8)),
                     bytes(rng.integers(0, 2, n, dtype=np.uint8)), b"\x05" * n):
            blk = _round_trip(data)
            if n < 13:  # under 13 bytes: one literal run
                assert blk == lc.seq(data)
    for name, data in lc.column_shapes().items():
        for n in (200, 4096, 65535, 65536, 65537, len(data)):
            _round_trip(data[:n])
    eq = _round_trip(b"\xab" * 100_000)
    assert len(eq) < 500
    _round_trip(bytes(rng.integers(0, 256, 100_000, dtype=np.uint8)))
    ids = lc.column_shapes()["ids"]
    assert len(_round_trip(ids)) < 0.7 * len(ids)


def test_encoder_keeps_the_end_of_block_rules():
    """Last 5 bytes literals, last match starting 12 bytes before the end:
    walk the sequences of blocks whose input would match to its last byte."""
    for n in (13, 14, 17, 18, 40, 1000):
        data = b"\x00" * n
        blk = cpp().lz4_compress_ref(data)
        p, d, last_match_start, last_lits = 0, 0, None, 0
        while True:
            token = blk[p]; p += 1
            ll = token >> 4
            if ll == 15:
                while True:
                    b = blk[p]; p += 1; ll += b
                    if b != 255:
                        break
            p += ll; d += ll
            if p == len(blk):
                last_lits = ll
                break
            p += 2
            ml = token & 15
            if ml == 15:
                while True:
                    b = blk[p]; p += 1; ml += b
                    if b != 255:
                        break
            last_match_start = d
            d += ml + 4
        assert d == n and last_lits >= 5
        assert last_match_start is not None and last_match_start <= n - 12


# ---- damaged blocks --------------------------------------------------- #

def _damage_target():
    data = bytearray(np.arange(70, dtype=np.int64).tobytes())
    rng = np.random.default_rng(2)
    for i in range(300, len(data), 7):
        data[i] = int(rng.integers(0, 256))
    while True:
        blk = CODEC.compress(bytes(data)).to_pybytes()
        if len(blk) <= 300:
            return blk, bytes(data)
        data = data[:-1]


def _liblz4_accepts(blk: bytes, n: int):
    """liblz4's bytes if it takes `blk` as an n-byte page, else None. It
    also succeeds on a block that decodes to fewer bytes, and pyarrow then
    hands back n bytes: the plain decoder tells those apart."""
    out = lc.liblz4_decode(blk, n)
    if out is None:
        return None
    try:
        if len(lc.decode(blk)) != n:
            return None
    except (IndexError, AssertionError):
        return None
    return out


def test_damaged_blocks():
    blk, orig = _damage_target()
    assert 250 <= len(blk) <= 300
    n = len(orig)
    assert cpp().lz4_block_decode_ref(blk, n) == orig
    refused = agreed = 0

    def check(bad):
        nonlocal refused, agreed
        got = cpp().lz4_block_decode_ref(bad, n)
        assert got is None or len(got) == n
        refused += got is None
        ref = _liblz4_accepts(bad, n)
        if ref is not None:
            assert got == ref
            agreed += 1

    for cut in range(len(blk)):
        check(blk[:cut])
    for i in range(len(blk)):
        for flip in (0x01, 0x80, 0xFF):
            bad = bytearray(blk)
            bad[i] ^= flip
            check(bytes(bad))
    rng = np.random.default_rng(3)
    for extra in range(1, 17):
        check(blk + bytes(rng.integers(0, 256, extra, dtype=np.uint8)))
    assert refused > len(blk)       # every truncation and more
    assert agreed > 100             # flips inside literals still decode


# ---- Hadoop framing (codec 5) ----------------------------------------- #

def _frame(data: bytes) -> bytes:
    blk = CODEC.compress(data).to_pybytes()
    return struct.pack(">II", len(data), len(blk)) + blk


def test_hadoop_framing():
    shapes = lc.column_shapes()
    a, b, c = shapes["ids"][:5000], shapes["i32small"][:777], shapes["f64"][:48]
    assert cpp().lz4_hadoop_decode_ref(_frame(a), len(a)) == a
    body = _frame(a) + _frame(b) + _frame(c)
    assert cpp().lz4_hadoop_decode_ref(body, len(a + b + c)) == a + b + c
    # a raw block under codec 5 (writers that never framed)
    raw = CODEC.compress(a).to_pybytes()
    assert cpp().lz4_hadoop_decode_ref(raw, len(a)) == a
    # sizes that do not add up, and nothing that decodes either way
    assert cpp().lz4_hadoop_decode_ref(body, len(a + b + c) + 1) is None
    assert cpp().lz4_hadoop_decode_ref(body[:-1], len(a + b + c)) is None
    assert cpp().lz4_hadoop_decode_ref(_frame(b""), 0) == b""


# ---- files ------------------------------------------------------------ #

N_ROWS = 6000


def _foreign_table():
    rng = np.random.default_rng(11)
    n = N_ROWS
    mask = rng.random(n) < 0.2
    schema = pa.schema([
        pa.field("id", pa.int64(), nullable=False),
        pa.field("f", pa.float64(), nullable=False),
        pa.field("ni", pa.int32()),
        pa.field("nf", pa.float32()),
        pa.field("s", pa.string()),
        pa.field("d", pa.int64()),
    ])
    return pa.table({
        "id": pa.array(np.arange(n, dtype=np.int64)),
        "f": pa.array(rng.normal(size=n)),
        "ni": pa.array(rng.integers(0, 100, n, dtype=np.int32), mask=mask),
        "nf": pa.array(rng.normal(size=n).astype(np.float32), mask=~mask),
        "s": pa.array([None if i % 11 == 0 else f"row-{i % 500}" for i in range(n)]),
        "d": pa.array(rng.integers(0, 20, n, dtype=np.int64) * 1000),
    }, schema=schema)


def _read_column_cpu(path, ci, field):
    import encoding_cases as ec

    if pa.types.is_string(field.type):
        return [None if v is None else v.decode()
                for v in ec.read_chunks_cpu_strings(path, ci)]
    data, valid = ec.read_chunks_cpu(path, ci, field.type.to_pandas_dtype())
    return [v if ok else None for v, ok in zip(data.tolist(), valid.tolist())]


@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_read_pyarrow_lz4_file(tmp_path, version):
    """pyarrow's compression="lz4" is codec 7: plain and dictionary pages,
    nullable columns, strings, v1 and v2 data pages."""
    tbl = _foreign_table()
    path = str(tmp_path / f"lz4_v{version}.parquet")
    pq.write_table(tbl, path, compression="lz4", use_dictionary=["s", "d"],
                   data_page_version=version, data_page_size=4096,
                   row_group_size=N_ROWS // 2)
    md = pq.ParquetFile(path).metadata
    assert md.row_group(0).column(0).compression == "LZ4"
    assert md.row_group(0).column(5).has_dictionary_page
    for ci, field in enumerate(tbl.schema):
        got = _read_column_cpu(path, ci, field)
        want = tbl.column(ci).to_pylist()
        if pa.types.is_floating(field.type):
            np.testing.assert_array_equal(
                np.array([np.nan if v is None else v for v in got]),
                np.array([np.nan if v is None else v for v in want]))
        else:
            assert got == want, field.name


def _register(t, path):
    from lakesoul_amd.meta.entities import (CommitOp, DataCommitInfo,
                                            DataFileOp, FileOp)

    t.client.commit_data_commit_info(DataCommitInfo(
        table_id=t.table_id, partition_desc="-5",
        file_ops=[DataFileOp(path, FileOp.add, 1)],
        commit_op=CommitOp.MergeCommit))


def test_cpu_scan_of_pyarrow_lz4_files(catalog):
    from lakesoul_amd.io.schema import Field, Schema

    t = catalog.create_table(
        "lz4foreign",
        Schema([Field("id", "int64", False), Field("f", "float64", False),
                Field("ni", "int32"), Field("nf", "float32"),
                Field("s", "string"), Field("d", "int64")]),
        primary_keys=["id"], hash_bucket_num=1)
    tbl = _foreign_table()
    p = f"{t.table_path}/part-extlz4000000000_0000.parquet"
    pq.write_table(tbl, p, compression="lz4", use_dictionary=["s", "d"],
                   data_page_size=4096, row_group_size=N_ROWS // 2)
    _register(t, p)
    got = t.scan(device="cpu").to_arrow().sort_by("id")
    assert got.num_rows == N_ROWS
    for name in tbl.column_names:
        assert got.column(name).to_pylist() == tbl.column(name).to_pylist(), name


def _native_data(n=20_000):
    rng = np.random.default_rng(5)
    return {
        "id": np.arange(n, dtype=np.int64),
        "v": rng.normal(size=n),
        "k": rng.integers(0, 100, n, dtype=np.int32),
        "s": [f"name-{i % 97}" for i in range(n)],
    }


def test_written_lz4_raw_table_is_read_by_pyarrow(catalog):
    from lakesoul_amd.io.schema import Field, Schema

    data = _native_data()
    for codec_name in ("lz4_raw", "lz4"):
        t = catalog.create_table(
            f"lz4native_{codec_name}",
            Schema([Field("id", "int64", False), Field("v", "float64", False),
                    Field("k", "int32"), Field("s", "string")]),
            primary_keys=["id"], hash_bucket_num=2,
            properties={"compression": codec_name})
        assert t.io_config().compression == codec_name
        t.upsert(data, device="cpu")
        files = [f.path for f in t.files()]
        assert files
        parts = []
        for f in files:
            md = pq.ParquetFile(f).metadata
            for rg in range(md.num_row_groups):
                for c in range(md.num_columns):
                    assert md.row_group(rg).column(c).compression == "LZ4", f
            parts.append(pq.read_table(f))
        got = pa.concat_tables(parts).sort_by("id")
        np.testing.assert_array_equal(got["id"].to_numpy(), data["id"])
        np.testing.assert_array_equal(got["v"].to_numpy(), data["v"])
        np.testing.assert_array_equal(got["k"].to_numpy(), data["k"])
        assert got["s"].to_pylist() == data["s"]
        # and by the project's own CPU scan
        back = t.scan(device="cpu").to_arrow().sort_by("id")
        np.testing.assert_array_equal(back["v"].to_numpy(), data["v"])
        assert back["s"].to_pylist() == data["s"]
        # compaction keeps the codec
        t.upsert({k: v[:100] for k, v in data.items()}, device="cpu")
        t.compaction(device="cpu")
        for f in t.files():
            md = pq.ParquetFile(f.path).metadata
            assert md.row_group(0).column(0).compression == "LZ4"
        assert t.scan(device="cpu").to_arrow().num_rows == len(data["id"])


def test_streaming_writer_lz4_raw(tmp_path, monkeypatch):
    from lakesoul_amd.io.batch import Batch
    from lakesoul_amd.io.multipart import StreamingParquetUpload
    from lakesoul_amd.io.schema import Field, Schema
    import lakesoul_amd.io.fs as fsmod

    root = tmp_path / "mockstore"
    root.mkdir()
    monkeypatch.setenv("LAKESOUL_MOCK_FS_ROOT", str(root))
    monkeypatch.setattr(fsmod, "_default_fs", None)
    schema = Schema([Field("id", "int64", False), Field("v", "float64"),
                     Field("s", "string")])
    n = 30_000
    rng = np.random.default_rng(6)
    v = rng.normal(size=n)
    b = Batch.from_dict({"id": np.arange(n, dtype=np.int64), "v": v,
                         "s": [f"s{i}" for i in range(n)]}, schema)
    up = StreamingParquetUpload("mock://data/part-lz4_0000.parquet", schema,
                                "lz4_raw", 1, row_group_size=10_000,
                                part_bytes=64 << 10)
    for i in range(3):
        up.write_batch(b.slice(i * 10_000, (i + 1) * 10_000))
    up.close()
    final = str(root / "data" / "part-lz4_0000.parquet")
    md = pq.ParquetFile(final).metadata
    assert md.num_row_groups == 3
    assert all(md.row_group(rg).column(c).compression == "LZ4"
               for rg in range(3) for c in range(3))
    got = pq.read_table(final)
    np.testing.assert_array_equal(got["id"].to_numpy(), np.arange(n))
    np.testing.assert_array_equal(got["v"].to_numpy(), v)
    assert got["s"].to_pylist() == [f"s{i}" for i in range(n)]


# ---- C ABI ------------------------------------------------------------ #

def test_c_writer_lz4_raw(lib, tmp_path):  # noqa: F811
    import ctypes

    lib.lakesoul_c_writer_set_compression.argtypes = [
        ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    path = str(tmp_path / "cw_lz4.parquet").encode()
    w = lib.lakesoul_c_writer_create(path)
    assert lib.lakesoul_c_writer_set_compression(ctypes.c_void_p(w), b"gzip", 0) == -1
    assert lib.lakesoul_c_writer_set_compression(ctypes.c_void_p(w), b"lz4", 0) == 0
    assert lib.lakesoul_c_writer_set_compression(ctypes.c_void_p(w), b"lz4_raw", 0) == 0
    tbl = pa.table({"id": pa.array(np.arange(3000, dtype=np.int64)),
                    "s": pa.array([f"x{i % 7}" for i in range(3000)])})
    schema_holder = ctypes.create_string_buffer(72)  # sizeof(ArrowSchema)
    tbl.schema._export_to_c(ctypes.addressof(schema_holder))
    assert lib.lakesoul_c_writer_set_schema(
        ctypes.c_void_p(w), ctypes.addressof(schema_holder)) == 0
    arr_holder = ctypes.create_string_buffer(80)  # sizeof(ArrowArray)
    tbl.to_batches()[0].to_struct_array()._export_to_c(ctypes.addressof(arr_holder))
    assert lib.lakesoul_c_writer_write(
        ctypes.c_void_p(w), ctypes.addressof(arr_holder)) == 0
    assert lib.lakesoul_c_writer_close(ctypes.c_void_p(w)) > 0
    md = pq.ParquetFile(path.decode()).metadata
    assert md.row_group(0).column(0).compression == "LZ4"
    got = pq.read_table(path.decode())
    np.testing.assert_array_equal(got["id"].to_numpy(), np.arange(3000))
    assert got["s"].to_pylist() == [f"x{i % 7}" for i in range(3000)]


# ---- sanitizers ------------------------------------------------------- #

def test_lz4_sanitizer_clean(tmp_path):
    """Decoder, encoder and Hadoop framing under AddressSanitizer + UBSan,
    input and output in exactly-sized heap buffers
    (csrc/cpp/tests/lz4_san.cc)."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "csrc", "cpp", "tests", "lz4_san.cc")
    exe = str(tmp_path / "lz4_san")
    cc = shutil.which("g++")
    if cc is None:
        pytest.skip("no g++")
    b = subprocess.run([cc, "-O1", "-g", "-std=c++17",
                        "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", src, "-o", exe],
                       capture_output=True, text=True)
    if b.returncode != 0:
        pytest.skip(f"sanitizer build unavailable: {b.stderr[-200:]}")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[:4000]
