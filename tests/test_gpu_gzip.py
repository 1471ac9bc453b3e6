"""GZIP pages on the GPU: the page kernel (csrc/hip/gzip.hip) on the corpus
of tests/gzip_corpus.py, and the scan route over pyarrow-written GZIP files
with LAKESOUL_GPU_GZIP=1 / 0 in fresh child processes. Only valid pages go
to the kernel: damaged ones are for its host twin and the sanitizer program
(test_gzip.py), which run the same parse and bounds code."""

import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import gzip_corpus as gc
from lz4_corpus import column_shapes
from test_gpu_lz4 import NAMES, REQUIRED_WIDTH, _columns, _expected, _table
from test_lz4 import _register

pytestmark = pytest.mark.gpu

GUARD = 64


def _launch_with_guards(entries):
    """All pages in one launch: sources back to back (so at every
    alignment), outputs at odd offsets between 0xA5 guards."""
    from lakesoul_amd.ops import hip

    src = bytearray(b"\x5a" * 3)
    jobs, doff = [], 1
    for _, page, orig in entries:
        doff += GUARD
        jobs.append([len(src), len(page), doff, len(orig)])
        src += page
        doff += len(orig) + GUARD
        doff += 1 - doff % 2  # odd
    total = doff + GUARD
    for so, sl, do, dl in jobs:  # the launch reads and writes inside both
        assert 0 <= so and so + sl <= len(src) and 0 <= do and do + dl <= total
    dst = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    status = hip().gzip_decompress_into(
        torch.frombuffer(src, dtype=torch.uint8).cuda(),
        torch.tensor(jobs, dtype=torch.int64).cuda(), dst)
    return jobs, status.cpu().numpy(), dst.cpu().numpy()


def test_kernel_on_corpus_with_guards():
    entries = gc.entries()
    jobs, status, out = _launch_with_guards(entries)
    assert (status == 0).all(), [(e[0], int(s)) for e, s in zip(entries, status) if s]
    covered = np.zeros(len(out), dtype=bool)
    for (name, _, orig), (_, _, do, dl) in zip(entries, jobs):
        assert out[do:do + dl].tobytes() == orig, name
        covered[do:do + dl] = True
        assert (out[do - GUARD:do] == 0xA5).all(), name
        assert (out[do + dl:do + dl + GUARD] == 0xA5).all(), name
    assert (out[~covered] == 0xA5).all()


def test_kernel_many_pages():
    """400 pages of 1 to 3000 bytes and 2100 of 1 to 40 bytes through the
    allocating binding: more pages than the grid's 2048 workgroups, so some
    workgroups decode a second page with the tables of the first in LDS."""
    from lakesoul_amd.ops import hip

    shapes = list(column_shapes().values())
    rng = np.random.default_rng(8)
    src, jobs, origs, doff = bytearray(), [], [], 0
    for p in range(2500):
        data = shapes[p % len(shapes)]
        n = int(rng.integers(1, 3000 if p < 400 else 41))
        start = int(rng.integers(0, len(data) - n))
        orig = data[start:start + n]
        strategy = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_DEFAULT_STRATEGY,
                    zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_RLE)[p % 5]
        page = gc.deflate(orig, level=(1, 6, 9)[p % 3], wbits=15 if p % 7 == 0 else 31,
                          strategy=strategy)
        jobs.append([len(src), len(page), doff, n])
        src += page
        doff += n
        origs.append(orig)
    assert len(jobs) > 2048
    dst, status = hip().gzip_decompress(
        torch.frombuffer(src, dtype=torch.uint8).cuda(),
        torch.tensor(jobs, dtype=torch.int64).cuda(), doff)
    assert (status.cpu().numpy() == 0).all()
    assert dst.cpu().numpy().tobytes() == b"".join(origs)


# ---- scan route ------------------------------------------------------- #

def _varint(buf, p):
    v = shift = 0
    while True:
        b = buf[p]
        p += 1
        v |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            return v, p


def _skip(buf, p, t):
    """Behind one thrift compact-protocol value of type t at buf[p]."""
    if t in (1, 2):
        return p
    if t == 3:
        return p + 1
    if t in (4, 5, 6):
        return _varint(buf, p)[1]
    if t == 7:
        return p + 8
    if t == 8:
        n, p = _varint(buf, p)
        return p + n
    if t in (9, 10):
        head = buf[p]
        p += 1
        n = head >> 4
        if n == 15:
            n, p = _varint(buf, p)
        for _ in range(n):
            p = _skip(buf, p, head & 15)
        return p
    if t == 12:
        return _struct(buf, p)[1]
    raise AssertionError(f"thrift type {t}")


def _struct(buf, p):
    """Top-level i32 fields {id: value} of the struct at buf[p], and where
    it ends."""
    fields, fid = {}, 0
    while True:
        head = buf[p]
        p += 1
        if head == 0:
            return fields, p
        if head >> 4:
            fid += head >> 4
        else:
            z, p = _varint(buf, p)
            fid = (z >> 1) ^ -(z & 1)
        t = head & 15
        if t == 5:
            z, p = _varint(buf, p)
            fields[fid] = (z >> 1) ^ -(z & 1)
        else:
            p = _skip(buf, p, t)


def _pages_of_required_columns(path):
    """(compressed, uncompressed) body sizes of every data page of the
    REQUIRED columns, walked from the page headers (PageHeader: 1 type,
    2 uncompressed_page_size, 3 compressed_page_size)."""
    buf = open(path, "rb").read()
    pf = pq.ParquetFile(path)
    md = pf.metadata
    pages = []
    for rg in range(md.num_row_groups):
        for c in range(md.num_columns):
            col = md.row_group(rg).column(c)
            if pf.schema.column(c).max_definition_level:
                continue
            assert col.compression == "GZIP" and not col.has_dictionary_page
            p, end = col.data_page_offset, col.data_page_offset + col.total_compressed_size
            while p < end:
                fields, body = _struct(buf, p)
                assert fields[1] == 0  # DATA_PAGE (v1)
                pages.append((fields[3], fields[2]))
                p = body + fields[3]
            assert p == end
    return pages


def _run_child(tmp_path, name, flag):
    out = tmp_path / f"child{flag}"
    out.mkdir()
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                         "gpu_gzip_child.py")
    env = dict(os.environ, LAKESOUL_GPU_GZIP=flag)
    r = subprocess.run(
        [sys.executable, child, str(out), str(tmp_path / "meta.db"),
         str(tmp_path / "wh"), name], env=env, capture_output=True, text=True,
        timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    info = json.load(open(out / "jobs.json"))
    assert info["flag"] == (flag == "1")
    return pa.ipc.open_file(str(out / "scan.arrow")).read_all(), info["jobs"]


def test_scan_route_foreign_files(catalog, tmp_path):
    """Two pyarrow-written GZIP files, a base and an upsert, 16 KB pages:
    scanned with the GPU route on and off, each in a fresh process."""
    t = _table(catalog, "gzipgpu_foreign")
    base = _columns(np.arange(20_000), 1)
    up = _columns(np.arange(0, 20_000, 4), 2)
    null_every = 9
    schema = pa.schema([
        pa.field("id", pa.int64(), nullable=False),
        pa.field("f", pa.float64(), nullable=False),
        pa.field("k", pa.int32(), nullable=False),
        pa.field("x", pa.float32(), nullable=False),
        pa.field("w", pa.int64(), nullable=False),
        pa.field("n", pa.float64()),
    ])
    pages = []
    for i, cols in enumerate((base, up)):
        arrays = {k: pa.array(v) for k, v in cols.items()}
        arrays["n"] = pa.array(cols["n"], mask=np.arange(len(cols["id"])) % null_every == 0)
        path = f"{t.table_path}/part-extgzipgpu00000{i}_0000.parquet"
        pq.write_table(pa.table(arrays, schema=schema), path, compression="gzip",
                       use_dictionary=False, data_page_size=16 << 10,
                       row_group_size=10_000)
        _register(t, path)
        pages += _pages_of_required_columns(path)
    rows = len(base["id"]) + len(up["id"])
    # several pages per chunk: 5 columns, 3 row groups, 2 to 5 pages each
    assert len(pages) >= 40 and sum(u for _, u in pages) == rows * REQUIRED_WIDTH

    on, jobs_on = _run_child(tmp_path, "gzipgpu_foreign", "1")
    off, jobs_off = _run_child(tmp_path, "gzipgpu_foreign", "0")
    # every page of the REQUIRED fixed-width columns, none left to the host
    assert sorted(map(tuple, jobs_on)) == sorted(pages)
    assert jobs_off == []
    assert on.equals(off)
    for name in NAMES:  # byte-identical, NaN payloads included
        a, b = on.column(name).combine_chunks(), off.column(name).combine_chunks()
        assert [x.to_pybytes() if x is not None else None for x in a.buffers()] == \
               [x.to_pybytes() if x is not None else None for x in b.buffers()], name
    cpu = t.scan(device="cpu").to_arrow().sort_by("id")
    on = on.sort_by("id")
    assert on.equals(cpu)
    want, valid = _expected(base, up, null_every)
    assert on.num_rows == len(base["id"])
    for name in NAMES[:-1]:
        np.testing.assert_array_equal(on[name].to_numpy(), want[name], name)
    got_n = on["n"].to_numpy(zero_copy_only=False)
    np.testing.assert_array_equal(np.isnan(got_n), ~valid)
    np.testing.assert_array_equal(got_n[valid], want["n"][valid])
