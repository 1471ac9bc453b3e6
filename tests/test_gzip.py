"""GZIP pages on the host: the DEFLATE decoder with gzip and zlib framing
(csrc/cpp/inflate.h) against zlib on the corpus of tests/gzip_corpus.py and
on damaged pages; pyarrow-written GZIP parquet files (codec 2) read column
by column, by the CPU scan and through the C ABI; the sanitizer program."""

import ctypes
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from lakesoul_amd.ops import cpp

import gzip_corpus as gc
from test_capi import lib  # noqa: F401  (the ctypes loader fixture)
from test_lz4 import N_ROWS, _foreign_table, _read_column_cpu, _register


def _by_name():
    return {n: (p, o) for n, p, o in gc.entries()}


# ---- decoder ---------------------------------------------------------- #

def test_decoder_on_corpus():
    names = set()
    for name, page, orig in gc.entries():
        names.add(name)
        assert gc.zlib_decode(page) == orig, name
        assert cpp().inflate_ref(page, len(orig)) == orig, name
        # the page's size is part of the question
        assert cpp().inflate_ref(page, len(orig) + 1) is None, name
        if orig:
            assert cpp().inflate_ref(page, len(orig) - 1) is None, name
    assert len(names) == len(gc.entries()) >= 70


def test_corpus_holds_what_it_is_built_for():
    e = _by_name()
    # block kinds by the first block's header bits (behind the 10-byte gzip
    # header): BTYPE is bits 1..2
    assert (e["ids_level0"][0][10] >> 1) & 3 == 0
    assert (e["ids_fixed"][0][10] >> 1) & 3 == 1
    assert (e["ids_level9"][0][10] >> 1) & 3 == 2
    assert e["ids_zlib"][0][:2] == b"\x78\x9c"
    # incompressible input: stored blocks of at most 65535 bytes, so several
    page, orig = e["random_200k"]
    assert len(page) > len(orig) and (page[10] >> 1) & 3 == 0
    # an empty stored block (00 00 ff ff) where the stream was flushed
    assert b"\x00\x00\xff\xff" in e["ids_sync_flush"][0]
    assert e["header_fields"][0][3] == 2 | 4 | 8 | 16
    assert e["two_members"][0].count(b"\x1f\x8b\x08") >= 2
    # zlib's encoder stops at distance 32506; the hand-assembled page goes
    # to 32768, and is about 100 KB
    assert 99_000 < len(e["hand_far_long_matches"][1]) < 101_000
    assert len(e["literals_64"][1]) == 64 and len(e["literals_65"][1]) == 65


def test_bare_deflate_streams():
    for raw in (gc.raw_15bit_code(), gc.raw_single_distance_code(),
                gc.raw_repeat_across_hlit()):
        want = zlib.decompressobj(-15).decompress(raw)
        assert want
        assert cpp().inflate_raw_ref(raw, len(want)) == want
        assert cpp().inflate_raw_ref(raw, len(want) + 1) is None
        assert cpp().inflate_raw_ref(raw + b"\x00", len(want)) is None
        # a bare stream is no page
        assert cpp().inflate_ref(raw, len(want)) is None


# ---- damaged pages ---------------------------------------------------- #

def _zlib_refuses_raw(raw: bytes) -> bool:
    try:
        d = zlib.decompressobj(-15)
        d.decompress(raw)
        return not d.eof
    except zlib.error:
        return True


def _refused(raw: bytes, n: int):
    """A bare stream and the gzip member around it are both refused (the
    member's CRC is that of n zero bytes: it is not what stops it)."""
    assert _zlib_refuses_raw(raw)
    assert cpp().inflate_raw_ref(raw, n) is None
    assert cpp().inflate_ref(gc.gzip_member(raw, b"\0" * n), n) is None


def test_every_truncation_is_refused():
    e = _by_name()
    small = [(n, *e[n]) for n in ("ids_200", "i32small_200", "hand_repeat_across_hlit",
                                  "hand_single_distance_code", "empty", "one_byte")]
    part = e["ids_200"][1]
    small.append(("zlib_200", gc.deflate(part, wbits=15), part))
    small.append(("stored_200", gc.deflate(part, 0), part))
    small.append(("two_members", gc.deflate(part[:40]) + gc.deflate(part[40:]), part))
    for name, page, orig in small:
        assert len(page) < 400
        assert cpp().inflate_ref(page, len(orig)) == orig, name
        for cut in range(len(page)):
            assert cpp().inflate_ref(page[:cut], len(orig)) is None, (name, cut)


def test_damaged_blocks_are_refused():
    e = _by_name()
    # LEN/NLEN mismatch: level 0 is one stored block behind the 10-byte header
    orig = e["ids_200"][1]
    page = bytearray(gc.deflate(orig, 0))
    assert page[10] == 1 and struct.unpack_from("<HH", page, 11) == (200, 200 ^ 0xFFFF)
    for at in (11, 12, 13, 14):
        bad = bytearray(page)
        bad[at] ^= 0x04
        assert cpp().inflate_ref(bytes(bad), len(orig)) is None, at

    # over-subscribed literal/length lengths: three codes of one bit
    w = gc.BitWriter()
    gc.dynamic_block(w, [(18, 97 - 11), (1, 0), (1, 0), (18, 138 - 11), (18, 19 - 11),
                         (1, 0), (0, 0)],
                     257, 1, [0] * 97 + [1, 1] + [0] * 157 + [1], [0], [97])
    _refused(w.to_bytes(), 1)
    # incomplete literal/length lengths: two codes of two bits
    w = gc.BitWriter()
    gc.dynamic_block(w, [(18, 97 - 11), (2, 0), (18, 138 - 11), (18, 20 - 11), (2, 0),
                         (0, 0)],
                     257, 1, [0] * 97 + [2] + [0] * 158 + [2], [0], [97])
    _refused(w.to_bytes(), 1)
    # incomplete distance lengths other than one 1-bit code: one 2-bit code
    w = gc.BitWriter()
    gc.dynamic_block(w, [(18, 97 - 11), (1, 0), (18, 138 - 11), (18, 20 - 11), (2, 0),
                         (2, 0), (2, 0)],
                     258, 1, [0] * 97 + [1] + [0] * 158 + [2, 2], [2], [97, (3, 1)])
    _refused(w.to_bytes(), 4)
    # over-subscribed code-length code: every one of the 19 has one bit
    w = gc.BitWriter()
    w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(15, 4)
    for _ in range(19):
        w.bits(1, 3)
    w.bits(0, 32)
    _refused(w.to_bytes(), 1)
    # a repeat with nothing before it, and one that runs past HLIT + HDIST
    w = gc.BitWriter()
    gc.dynamic_block(w, [(16, 0), (18, 138 - 11), (18, 116 - 11), (1, 0), (1, 0)],
                     257, 1, [0] * 256 + [1], [1], [])
    _refused(w.to_bytes(), 0)
    w = gc.BitWriter()
    gc.dynamic_block(w, [(18, 97 - 11), (1, 0), (18, 138 - 11), (18, 20 - 11), (1, 0),
                         (18, 0)],
                     257, 1, [0] * 97 + [1] + [0] * 158 + [1], [0], [97])
    _refused(w.to_bytes(), 1)
    # literal/length symbol 286 (it has a code in the fixed block)
    w = gc.BitWriter()
    gc.fixed_block(w, [97, 286, 97])
    _refused(w.to_bytes(), 2)
    # distance code 30
    fixed_lit = gc.canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
    w = gc.BitWriter()
    w.bits(1, 1); w.bits(1, 2)
    w.code(*fixed_lit[97]); w.code(*fixed_lit[257]); w.code(30, 5)
    w.code(*fixed_lit[256])
    _refused(w.to_bytes(), 4)
    # a distance beyond the output so far
    w = gc.BitWriter()
    gc.fixed_block(w, [97, 98, (3, 3)])
    _refused(w.to_bytes(), 5)
    # ... also in the second member: distances do not reach into the first
    w = gc.BitWriter()
    gc.fixed_block(w, [97, (3, 2)])
    first = gc.deflate(b"abcdefgh")
    assert cpp().inflate_ref(first + gc.gzip_member(w.to_bytes(), b"aaaa"), 12) is None
    # block type 3
    _refused(b"\x07\x00", 0)
    # no end-of-block code among the lengths
    w = gc.BitWriter()
    gc.dynamic_block(w, [(18, 97 - 11), (1, 0), (1, 0), (18, 138 - 11), (18, 20 - 11),
                         (0, 0)],
                     257, 1, [0] * 97 + [1, 1] + [0] * 157 + [1], [0], [97])
    _refused(w.to_bytes()[:-1] + b"\x00" * 8, 1)


def test_damaged_framing_is_refused():
    e = _by_name()
    page, orig = e["i32small_200"]
    n = len(orig)
    assert cpp().inflate_ref(page, n) == orig
    # output longer and shorter than n (test_decoder_on_corpus does it for
    # every entry); a stream that decodes to more than fits
    assert cpp().inflate_ref(page, n - 1) is None
    assert cpp().inflate_ref(page, n + 1) is None
    assert cpp().inflate_ref(page, 0) is None
    # CRC32 off by one bit, ISIZE off by one
    for at in range(len(page) - 8, len(page) - 4):
        for bit in (1, 0x80):
            bad = bytearray(page)
            bad[at] ^= bit
            assert cpp().inflate_ref(bytes(bad), n) is None
    for delta in (1, -1):
        bad = page[:-4] + struct.pack("<I", n + delta)
        assert cpp().inflate_ref(bad, n) is None
        assert cpp().inflate_ref(bad, n + delta) is None
    # trailing garbage that is not a member
    for tail in (b"\x00", b"\x1f", b"\x1f\x8b", b"\x1f\x8b\x08\x00", b"garbage!" * 4,
                 page[:-1]):
        assert cpp().inflate_ref(page + tail, n) is None, tail
        assert cpp().inflate_ref(page + tail, 2 * n) is None, tail
    assert cpp().inflate_ref(page + page, 2 * n) == orig + orig
    # header: magic, method, reserved flag bits
    for at, v in ((0, 0x1e), (1, 0x8a), (2, 7), (3, 0x20), (3, 0x80)):
        bad = bytearray(page)
        bad[at] = v
        assert cpp().inflate_ref(bytes(bad), n) is None, at
    # zlib framing: Adler-32, header check, preset dictionary, trailing byte
    zp = gc.deflate(orig, wbits=15)
    assert cpp().inflate_ref(zp, n) == orig
    for at in range(len(zp) - 4, len(zp)):
        bad = bytearray(zp)
        bad[at] ^= 1
        assert cpp().inflate_ref(bytes(bad), n) is None
    assert cpp().inflate_ref(b"\x78\x9d" + zp[2:], n) is None
    assert cpp().inflate_ref(b"\x78\xbb" + zp[2:], n) is None  # FDICT, check ok
    assert (0x78bb % 31) == 0
    assert cpp().inflate_ref(zp + b"\x00", n) is None
    assert cpp().inflate_ref(b"", 0) is None
    assert cpp().inflate_ref(b"\x1f", 0) is None


FLIPS = 600
FLIP_SEED = 21


def test_flipped_bytes():
    """Single-byte damage: never a crash; whatever is accepted is what zlib
    makes of the same bytes. zlib must refuse at least 90 % of the flips, so
    that the test does not pass on damage to the unused header bytes only."""
    e = _by_name()
    rng = np.random.default_rng(FLIP_SEED)
    for name in ("i32small_4096", "hand_15bit_code"):
        page, orig = e[name]
        n = len(orig)
        accepted = zlib_accepted = 0
        for _ in range(FLIPS):
            bad = bytearray(page)
            at = int(rng.integers(0, len(page)))
            bad[at] ^= int(rng.integers(1, 256))
            bad = bytes(bad)
            got = cpp().inflate_ref(bad, n)
            ref = gc.zlib_decode(bad)
            if ref is not None and len(ref) != n:
                ref = None
            zlib_accepted += ref is not None
            if got is not None:
                accepted += 1
                assert got == ref, (name, at)
        print(f"{name}: {len(page)} bytes, {FLIPS} flips, accepted {accepted}, "
              f"zlib accepted {zlib_accepted}")
        assert zlib_accepted <= FLIPS // 10, (name, zlib_accepted)
        assert accepted <= zlib_accepted


# ---- files ------------------------------------------------------------ #

@pytest.mark.parametrize("version", ["1.0", "2.0"])
def test_read_pyarrow_gzip_file(tmp_path, version):
    """pyarrow's compression="gzip" is codec 2: plain and dictionary pages,
    nullable columns, strings, v1 and v2 data pages, two row groups."""
    tbl = _foreign_table()
    path = str(tmp_path / f"gzip_v{version}.parquet")
    pq.write_table(tbl, path, compression="gzip", use_dictionary=["s", "d"],
                   data_page_version=version, data_page_size=4096,
                   row_group_size=N_ROWS // 2)
    md = pq.ParquetFile(path).metadata
    assert md.num_row_groups == 2
    assert md.row_group(0).column(0).compression == "GZIP"
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


def _gzip_foreign(catalog, name):
    from lakesoul_amd.io.schema import Field, Schema

    t = catalog.create_table(
        name,
        Schema([Field("id", "int64", False), Field("f", "float64", False),
                Field("ni", "int32"), Field("nf", "float32"),
                Field("s", "string"), Field("d", "int64")]),
        primary_keys=["id"], hash_bucket_num=1)
    tbl = _foreign_table()
    p = f"{t.table_path}/part-extgzip00000000_0000.parquet"
    pq.write_table(tbl, p, compression="gzip", use_dictionary=["s", "d"],
                   data_page_size=4096, row_group_size=N_ROWS // 2)
    assert pq.ParquetFile(p).metadata.row_group(1).column(4).compression == "GZIP"
    _register(t, p)
    return t, tbl, p


def test_cpu_scan_of_pyarrow_gzip_files(catalog):
    t, tbl, _ = _gzip_foreign(catalog, "gzipforeign")
    got = t.scan(device="cpu").to_arrow().sort_by("id")
    assert got.num_rows == N_ROWS
    for name in tbl.column_names:
        assert got.column(name).to_pylist() == tbl.column(name).to_pylist(), name


def test_gzip_is_not_written():
    """Read only: the writers' codec names gain no value."""
    from lakesoul_amd.io import multipart, writer

    assert "gzip" not in writer._CODEC_ID and 2 not in writer._CODEC_ID.values()
    assert "gzip" not in multipart._CODEC_ID and 2 not in multipart._CODEC_ID.values()


# ---- C ABI ------------------------------------------------------------ #

def test_c_reader_gzip_file(lib, catalog):  # noqa: F811
    _, tbl, path = _gzip_foreign(catalog, "gzipcabi")
    vp = ctypes.c_void_p
    r = lib.lakesoul_c_reader_create()
    lib.lakesoul_c_reader_add_file(vp(r), path.encode())
    lib.lakesoul_c_reader_add_primary_key(vp(r), b"id")
    lib.lakesoul_c_reader_set_batch_size(vp(r), 1024)
    assert lib.lakesoul_c_reader_start(vp(r)) == 0, lib.lakesoul_c_last_error()
    schema_holder = ctypes.create_string_buffer(72)  # sizeof(ArrowSchema)
    assert lib.lakesoul_c_reader_schema(vp(r), ctypes.addressof(schema_holder)) == 0
    schema = pa.Schema._import_from_c(ctypes.addressof(schema_holder))
    assert [f.name for f in schema] == tbl.column_names
    rows = []
    while True:
        arr_holder = ctypes.create_string_buffer(80)  # sizeof(ArrowArray)
        rc = lib.lakesoul_c_reader_next(vp(r), ctypes.addressof(arr_holder))
        assert rc >= 0, lib.lakesoul_c_last_error()
        if rc == 0:
            break
        sa = pa.Array._import_from_c(ctypes.addressof(arr_holder),
                                     pa.struct(list(schema)))
        rows.append(pa.RecordBatch.from_struct_array(sa))
    lib.lakesoul_c_reader_close(vp(r))
    got = pa.Table.from_batches(rows).sort_by("id")
    assert got.num_rows == N_ROWS
    for name in tbl.column_names:
        assert got.column(name).to_pylist() == tbl.column(name).to_pylist(), name


# ---- sanitizers ------------------------------------------------------- #

def test_gzip_sanitizer_clean(tmp_path):
    """inflate_page and inflate_raw under AddressSanitizer + UBSan, input
    and output in exactly-sized heap buffers
    (csrc/cpp/tests/inflate_san.cc)."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "csrc", "cpp", "tests", "inflate_san.cc")
    exe = str(tmp_path / "inflate_san")
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
