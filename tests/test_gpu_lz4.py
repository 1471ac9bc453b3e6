"""LZ4_RAW pages on the GPU: the page kernel (csrc/hip/lz4.hip) on the
corpus of tests/lz4_corpus.py, and the scan route over pyarrow-written and
project-written LZ4_RAW files. Only valid blocks go to the kernel: damaged
ones are for its host twin and the sanitizer program (test_lz4.py), which
run the same parse and bounds code."""

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import lz4_corpus as lc

pytestmark = pytest.mark.gpu

GUARD = 64


def _launch_with_guards(entries):
    """All blocks in one launch: sources back to back (so at every
    alignment), outputs at odd offsets between 0xA5 guards."""
    from lakesoul_amd.ops import hip

    src = bytearray(b"\x5a" * 3)
    jobs, doff = [], 1
    for _, block, orig in entries:
        doff += GUARD
        jobs.append([len(src), len(block), doff, len(orig)])
        src += block
        doff += len(orig) + GUARD
        doff += 1 - doff % 2  # odd
    total = doff + GUARD
    for so, sl, do, dl in jobs:  # the launch reads and writes inside both
        assert 0 <= so and so + sl <= len(src) and 0 <= do and do + dl <= total
    dst = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    status = hip().lz4_decompress_into(
        torch.frombuffer(src, dtype=torch.uint8).cuda(),
        torch.tensor(jobs, dtype=torch.int64).cuda(), dst)
    return jobs, status.cpu().numpy(), dst.cpu().numpy()


def test_kernel_on_corpus_with_guards():
    entries = lc.entries()
    jobs, status, out = _launch_with_guards(entries)
    assert (status == 0).all(), [e[0] for e, s in zip(entries, status) if s]
    covered = np.zeros(len(out), dtype=bool)
    for (name, _, orig), (_, _, do, dl) in zip(entries, jobs):
        assert out[do:do + dl].tobytes() == orig, name
        covered[do:do + dl] = True
        assert (out[do - GUARD:do] == 0xA5).all(), name
        assert (out[do + dl:do + dl + GUARD] == 0xA5).all(), name
    assert (out[~covered] == 0xA5).all()


def test_kernel_many_pages():
    """About 400 small real blocks through the allocating binding: more
    pages than one pass of a small grid, every page its own wave."""
    from lakesoul_amd.ops import hip

    codec = pa.Codec("lz4_raw")
    shapes = list(lc.column_shapes().values())
    rng = np.random.default_rng(8)
    src, jobs, origs, doff = bytearray(), [], [], 0
    for p in range(400):
        data = shapes[p % len(shapes)]
        n = int(rng.integers(1, 3000))
        start = int(rng.integers(0, len(data) - n))
        orig = data[start:start + n]
        block = codec.compress(orig).to_pybytes()
        jobs.append([len(src), len(block), doff, n])
        src += block
        doff += n
        origs.append(orig)
    dst, status = hip().lz4_decompress(
        torch.frombuffer(src, dtype=torch.uint8).cuda(),
        torch.tensor(jobs, dtype=torch.int64).cuda(), doff)
    assert (status.cpu().numpy() == 0).all()
    assert dst.cpu().numpy().tobytes() == b"".join(origs)


# ---- scan route ------------------------------------------------------- #

REQUIRED_WIDTH = 8 + 8 + 4 + 4 + 8  # id, f, k, x, w
NAMES = ["id", "f", "k", "x", "w", "n"]


def _columns(ids, seed):
    rng = np.random.default_rng(seed)
    m = len(ids)
    return {
        "id": ids.astype(np.int64),
        "f": rng.normal(size=m),
        "k": rng.integers(0, 100, m, dtype=np.int32),
        "x": rng.normal(size=m).astype(np.float32),
        "w": rng.integers(0, 10**12, m, dtype=np.int64),
        "n": rng.normal(size=m),
    }


def _table(catalog, name, **kw):
    from lakesoul_amd.io.schema import Field, Schema

    return catalog.create_table(
        name,
        Schema([Field("id", "int64", False), Field("f", "float64", False),
                Field("k", "int32", False), Field("x", "float32", False),
                Field("w", "int64", False), Field("n", "float64")]),
        primary_keys=["id"], hash_bucket_num=1, **kw)


def _expected(base, up, null_every):
    out = {k: v.copy() for k, v in base.items()}
    valid = np.arange(len(base["id"])) % null_every != 0
    up_valid = np.arange(len(up["id"])) % null_every != 0
    for k in out:
        out[k][up["id"]] = up[k]
    valid[up["id"]] = up_valid
    return out, valid


def _check_scan_route(t, files, base, up, null_every, min_jobs, monkeypatch):
    from lakesoul_amd.io import reader_gpu

    rows = len(base["id"]) + len(up["id"])
    monkeypatch.setattr(reader_gpu, "_GPU_LZ4", True)
    raw = reader_gpu.fetch_raw(files, NAMES)
    jobs = raw["lz4_jobs"].view(-1, 4)
    # every page of the REQUIRED fixed-width columns, none left to the host
    assert int(jobs[:, 3].sum()) == rows * REQUIRED_WIDTH
    assert jobs.shape[0] >= min_jobs
    on = t.scan(device="cuda").to_arrow()
    monkeypatch.setattr(reader_gpu, "_GPU_LZ4", False)
    assert reader_gpu.fetch_raw(files, NAMES)["lz4_jobs"].numel() == 0
    off = t.scan(device="cuda").to_arrow()
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


def test_scan_route_foreign_files(catalog, monkeypatch):
    """Two pyarrow-written LZ4 files, a base and an upsert, 16 KB pages."""
    from test_lz4 import _register

    t = _table(catalog, "lz4gpu_foreign")
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
    files = []
    for i, cols in enumerate((base, up)):
        arrays = {k: pa.array(v) for k, v in cols.items()}
        arrays["n"] = pa.array(cols["n"], mask=np.arange(len(cols["id"])) % null_every == 0)
        path = f"{t.table_path}/part-extlz4gpu000000{i}_0000.parquet"
        pq.write_table(pa.table(arrays, schema=schema), path, compression="lz4",
                       use_dictionary=False, data_page_size=16 << 10,
                       row_group_size=10_000)
        assert pq.ParquetFile(path).metadata.row_group(0).column(0).compression == "LZ4"
        _register(t, path)
        files.append(path)
    # several pages per chunk: 5 columns, 3 row groups, 2 to 5 pages each
    _check_scan_route(t, files, base, up, null_every, 40, monkeypatch)


def test_scan_route_native_files(catalog, monkeypatch):
    """The same for files the project writes with compression="lz4_raw"."""
    t = _table(catalog, "lz4gpu_native", properties={"compression": "lz4_raw"})
    base = _columns(np.arange(20_000), 3)
    up = _columns(np.arange(0, 20_000, 4), 4)
    null_every = 7
    for cols in (base, up):
        data = {k: pa.array(v) for k, v in cols.items()}
        data["n"] = pa.array(cols["n"], mask=np.arange(len(cols["id"])) % null_every == 0)
        t.upsert(pa.table(data), device="cuda")
    files = [f.path for f in t.files()]
    assert len(files) == 2
    for f in files:
        assert pq.ParquetFile(f).metadata.row_group(0).column(0).compression == "LZ4"
    _check_scan_route(t, files, base, up, null_every, 10, monkeypatch)
