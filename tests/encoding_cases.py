"""Shared inputs and readers of test_parquet_encodings.py (CPU) and
test_gpu_encodings.py (GPU): pyarrow-written DELTA_BINARY_PACKED,
BYTE_STREAM_SPLIT, DELTA_LENGTH_BYTE_ARRAY and DELTA_BYTE_ARRAY files.

Row counts sit on the block layout's boundaries. pyarrow writes INT64
pages as 256-value blocks of 4 miniblocks (64 values each) and INT32 pages
as 128 / 4 (32 each); the first value lives in the header, so 65 int64
values are one full miniblock, 66 add a padded one, 257 are one full
block and 258 add a second block with a single live miniblock."""

import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

INT64_COUNTS = [1, 2, 64, 65, 66, 257, 258]
INT32_COUNTS = [1, 33, 34, 129, 130]
BSS_COUNTS = [1, 63, 64, 65]

# 5000 rows in pages of ~64 values and row groups of 2000: several pages
# per chunk, three chunks
MULTI_N = 5000
MULTI_KW = dict(data_page_size=512, write_batch_size=64, row_group_size=2000)

VERSIONS = ["1.0", "2.0"]
CODECS = ["none", "zstd", "snappy"]


def int_value_sets(np_dtype, n, seed=0):
    """name -> n values: tiny widths, width 0, widths growing per
    miniblock, a full-width miniblock ([0, MAX]: deltas +MAX, -MAX, so
    delta - min_delta needs all 64 / 32 bits), wraparound ([MIN, MAX]:
    both deltas wrap to -1 / +1, width 2), and the full range."""
    info = np.iinfo(np_dtype)
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    return {
        "arange": i.astype(np_dtype),
        "const": np.full(n, 7, dtype=np_dtype),
        "squares": (i * i * (1000 if info.bits == 64 else 1)).astype(np_dtype),
        "fullwidth": np.array([0, info.max] * n, dtype=np_dtype)[:n],
        "wrap": np.array([info.min, info.max] * n, dtype=np_dtype)[:n],
        "random": rng.integers(info.min, info.max, n, dtype=np_dtype,
                               endpoint=True),
    }


def float_specials(np_dtype, n, seed=0):
    """Random floats with NaNs that carry payload bits, both zeros and
    both infinities up front (as many as fit in n)."""
    rng = np.random.default_rng(seed)
    udt = np.uint32 if np.dtype(np_dtype).itemsize == 4 else np.uint64
    if udt is np.uint32:
        nan_bits = [0x7FC00001, 0xFFC12345, 0x7F800001]
    else:
        nan_bits = [0x7FF8000000000001, 0xFFF8123456789ABC, 0x7FF0000000000001]
    special = np.concatenate([
        np.array(nan_bits, dtype=udt).view(np_dtype),
        np.array([0.0, -0.0, np.inf, -np.inf], dtype=np_dtype)])
    out = rng.normal(size=n).astype(np_dtype)
    k = min(n, len(special))
    out[:k] = special[:k]
    return out


def null_mask(n, kind, seed=0):
    """True = null. 'some': ~30 % nulls; 'all': every row; 'page': rows
    2000..3999 (with MULTI_KW the whole second row group, so each of its
    pages is entirely null) plus ~30 % elsewhere."""
    rng = np.random.default_rng(seed + 17)
    if kind == "all":
        return np.ones(n, dtype=bool)
    m = rng.random(n) < 0.3
    if kind == "page":
        assert n >= 4000
        m[2000:4000] = True
    return m


def bits(a):
    """Integer view of a numeric array: NaN payloads and -0.0 count."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)
    return a


def write(path, columns, encodings, version="1.0", codec="none", **kw):
    """columns: name -> pyarrow array. Dictionary off, each column in its
    listed encoding (others PLAIN). Returns the path as str; asserts the
    file really carries the encodings asked for."""
    path = str(path)
    tbl = pa.table(columns)
    pq.write_table(tbl, path, use_dictionary=False, column_encoding=encodings,
                   data_page_version=version, compression=codec, **kw)
    md = pq.ParquetFile(path).metadata
    names = list(columns)
    for rg in range(md.num_row_groups):
        for name, enc in encodings.items():
            got = md.row_group(rg).column(names.index(name)).encodings
            assert enc in got, (name, enc, got)
    return path


def multi_columns(null_kind):
    """The multi-page, multi-chunk case: name -> (values, null mask or None)
    and name -> encoding. null_kind 'page' adds ~30 % nulls, an entirely
    null row group and an entirely null column."""
    n = MULTI_N
    values = {
        "a": int_value_sets(np.int64, n, 1)["random"],
        "b": int_value_sets(np.int32, n, 2)["random"],
        "sorted": np.cumsum(np.random.default_rng(3).integers(0, 1000, n)).astype(np.int64),
        "f": float_specials(np.float64, n, 4),
        "g": float_specials(np.float32, n, 5),
    }
    cols = {k: (v, null_mask(n, null_kind, 11 + i) if null_kind else None)
            for i, (k, v) in enumerate(values.items())}
    encs = {"a": "DELTA_BINARY_PACKED", "b": "DELTA_BINARY_PACKED",
            "sorted": "DELTA_BINARY_PACKED", "f": "BYTE_STREAM_SPLIT",
            "g": "BYTE_STREAM_SPLIT"}
    if null_kind:
        cols["allnull"] = (np.zeros(n, dtype=np.int64), null_mask(n, "all"))
        encs["allnull"] = "DELTA_BINARY_PACKED"
    return cols, encs


def write_dict_fallback(path, codec="none"):
    """A file whose dictionary overflows: row group 0 (few distinct values)
    stays dictionary-encoded, row group 1 starts with dictionary pages and
    falls back to PLAIN pages. pyarrow cannot combine a dictionary with a
    DELTA_* fallback, so PLAIN stands in for the fallback encoding; the
    reader turns the index pages into values in the same way. Returns
    (path, int64 values, list of str)."""
    n = 20000
    rng = np.random.default_rng(21)
    a = np.concatenate([rng.integers(0, 50, n // 2),
                        rng.integers(0, 2**40, n // 2)]).astype(np.int64)
    s = [f"v{x:x}" for x in a]
    path = str(path)
    pq.write_table(pa.table({"a": pa.array(a), "s": pa.array(s)}), path,
                   use_dictionary=True, dictionary_pagesize_limit=4096,
                   data_page_size=2048, row_group_size=n // 2, compression=codec)
    md = pq.ParquetFile(path).metadata
    assert md.num_row_groups == 2
    for c in range(2):
        for rg in range(2):
            col = md.row_group(rg).column(c)
            assert col.has_dictionary_page and "RLE_DICTIONARY" in col.encodings
    return path, a, s


# ---- readers ---------------------------------------------------------- #

def read_chunks_cpu(path, col_index, np_dtype):
    """Column through cpp().read_chunk_cpu, row groups concatenated:
    (full-length values, valid bool)."""
    from lakesoul_amd.ops import cpp

    nrg = pq.ParquetFile(path).metadata.num_row_groups
    h = cpp().open_parquet(path)
    try:
        data, valid = [], []
        for rg in range(nrg):
            d = cpp().read_chunk_cpu(h, rg, col_index)
            data.append(d["data"].numpy().view(np_dtype))
            v = d["validity"].numpy()
            valid.append(v.astype(bool) if len(v)
                         else np.ones(d["num_values"], dtype=bool))
    finally:
        cpp().close_parquet(h)
    return np.concatenate(data), np.concatenate(valid)


def read_chunks_cpu_strings(path, col_index):
    """String column through cpp().read_chunk_cpu as a list of bytes/None."""
    from lakesoul_amd.ops import cpp

    nrg = pq.ParquetFile(path).metadata.num_row_groups
    h = cpp().open_parquet(path)
    out = []
    try:
        for rg in range(nrg):
            d = cpp().read_chunk_cpu(h, rg, col_index)
            offs = d["offsets"].numpy()
            by = d["bytes"].numpy().tobytes()
            v = d["validity"].numpy()
            for i in range(d["num_values"]):
                if len(v) and not v[i]:
                    out.append(None)
                else:
                    out.append(by[offs[i]:offs[i + 1]])
    finally:
        cpp().close_parquet(h)
    return out


def unit_valid(raw, u):
    from lakesoul_amd.ops import cpp

    d = raw["desc"][u]
    nv, voff = int(d[cpp().UD_NUM_VALUES]), int(d[cpp().UD_VALIDITY_OFF])
    if voff < 0:
        return np.ones(nv, dtype=bool)
    return raw["validity"].numpy()[voff:voff + nv].astype(bool)


def unit_plain_column(raw, u, np_dtype):
    """Host-route fixed-width unit column u: (dense stored values, valid)."""
    from lakesoul_amd.ops import cpp

    d = raw["desc"][u]
    assert int(d[cpp().UD_ENC]) == 0
    off, ln = int(d[cpp().UD_VAL_OFF]), int(d[cpp().UD_VAL_LEN])
    return (raw["values"].numpy()[off:off + ln].view(np_dtype),
            unit_valid(raw, u))


def unit_string_column(raw, u):
    """Unit string column u as a list of bytes/None."""
    from lakesoul_amd.ops import cpp

    d = raw["desc"][u]
    nv = int(d[cpp().UD_NUM_VALUES])
    so = int(d[cpp().UD_SOFF_OFF])
    offs = raw["soffs"].numpy()[so:so + nv + 1]
    b0, bl = int(d[cpp().UD_SBYTES_OFF]), int(d[cpp().UD_SBYTES_LEN])
    by = raw["values"].numpy()[b0:b0 + bl].tobytes()
    valid = unit_valid(raw, u)
    return [by[offs[i]:offs[i + 1]] if valid[i] else None for i in range(nv)]


def read_unit_host(paths, names):
    """read_unit_raw with the host route (the 4-argument call)."""
    from lakesoul_amd.ops import cpp

    return cpp().read_unit_raw([str(p) for p in paths], names, 0, False)


def read_unit_gpu_route(paths, names):
    """read_unit_raw that keeps DELTA_BINARY_PACKED / BYTE_STREAM_SPLIT
    pages raw for the GPU kernels."""
    from lakesoul_amd.ops import cpp

    return cpp().read_unit_raw([str(p) for p in paths], names, 0, False,
                               gpu_delta=True)


def string_sets(n=300):
    """name -> list of str: empty strings, one 5000-byte value, sorted keys
    with long shared prefixes, non-ASCII text."""
    keys = sorted(f"tenant-0001/region-eu-west/bucket-{i // 7:05d}/key-{i:07d}"
                  for i in range(n))
    return {
        "empty": [""] * 5,
        "mixed_empty": ["", "a", "", "bc", ""] * 13,
        "big": ["x", "y" * 5000, "z"],
        "prefix": keys,
        "unicode": [("héllo-wörld-" if i % 2 else "数据湖-") + f"{i:04d}-Ω"
                    for i in range(n)],
    }


def commit_foreign(table, path):
    """Commit a foreign parquet file into bucket 0 of `table`."""
    from lakesoul_amd.meta.entities import (CommitOp, DataCommitInfo,
                                            DataFileOp, FileOp)

    table.client.commit_data_commit_info(DataCommitInfo(
        table_id=table.table_id, partition_desc="-5",
        file_ops=[DataFileOp(path, FileOp.add, os.path.getsize(path))],
        commit_op=CommitOp.MergeCommit,
    ))


def mk_catalog(tmp_path):
    from lakesoul_amd.meta.client import MetaClient
    from lakesoul_amd.meta.store import SqliteMetaStore
    from lakesoul_amd.tables.catalog import LakeSoulCatalog

    store = SqliteMetaStore(str(tmp_path / "meta.db"))
    return LakeSoulCatalog(MetaClient(store), warehouse=str(tmp_path / "wh"))


def foreign_table(tmp_path, catalog, pks, name="foreign_enc", properties=None,
                  c_nulls=True):
    """A PK table with an upsert of ours (rows 0..n) and a committed foreign
    file (rows 0..m and n..n+100, every column in a v2 encoding, nulls in
    the value columns unless c_nulls is off). Returns (table, the frame a
    UseLast scan must give, (foreign ids, foreign c, c null mask))."""
    import pandas as pd

    from lakesoul_amd.io.schema import Field, Schema

    t = catalog.create_table(
        name,
        Schema([Field("id", "int64", False), Field("id2", "int32", False),
                Field("c", "int64"), Field("v", "float64"), Field("s", "string")]),
        primary_keys=pks, hash_bucket_num=1, properties=properties or {},
    )
    n, m = 3000, 700
    ids = np.arange(n, dtype=np.int64)
    t.upsert({"id": ids, "id2": (ids % 5).astype(np.int32),
              "c": np.ones(n, dtype=np.int64), "v": np.zeros(n),
              "s": ["ours"] * n}, device="cpu")
    fid = np.concatenate([np.arange(m), np.arange(n, n + 100)]).astype(np.int64)
    k = len(fid)
    rng = np.random.default_rng(8)
    fc = rng.integers(-10**12, 10**12, k).astype(np.int64)
    fv = float_specials(np.float64, k, 2)
    fv[:3] = [1.5, 2.5, 3.5]   # keep NaNs out of row-wise frame compares
    fs = [f"theirs/shared-prefix/{i:06d}" for i in range(k)]
    cmask = null_mask(k, "some", 1) if c_nulls else np.zeros(k, dtype=bool)
    smask = null_mask(k, "some", 2)
    foreign = write(
        tmp_path / "part-foreign0000000_0000.parquet",
        {"id": pa.array(fid), "id2": pa.array((fid % 5).astype(np.int32)),
         "c": pa.array(fc, mask=cmask), "v": pa.array(fv),
         "s": pa.array(fs, type=pa.string(), mask=smask)},
        {"id": "DELTA_BINARY_PACKED", "id2": "DELTA_BINARY_PACKED",
         "c": "DELTA_BINARY_PACKED", "v": "BYTE_STREAM_SPLIT",
         "s": "DELTA_BYTE_ARRAY"},
        "2.0", "zstd", data_page_size=2048, write_batch_size=128)
    commit_foreign(t, foreign)
    exp = pd.DataFrame({
        "id": np.concatenate([ids, fid[m:]]),
        "id2": np.concatenate([ids % 5, fid[m:] % 5]).astype(np.int32),
        "c": np.concatenate([np.ones(n), np.zeros(100)]),
        "v": np.zeros(n + 100), "s": ["ours"] * (n + 100)})
    exp["c"] = exp["c"].astype("float64")
    order = fid  # the frame's row index is the id
    exp.loc[order, "c"] = np.where(cmask, np.nan, fc.astype(np.float64))
    exp.loc[order, "v"] = fv
    exp["s"] = exp["s"].astype(object)
    exp.loc[order, "s"] = [None if smask[i] else fs[i] for i in range(k)]
    return t, exp, (fid, fc, cmask)


def frame_bits(df):
    """Row-sorted frame with floats as integer bit patterns and nulls as
    None, for exact comparison."""
    df = df.sort_values("id").reset_index(drop=True)
    out = {}
    for c in df.columns:
        col = df[c]
        if col.dtype.kind == "f":
            out[c] = col.to_numpy().view(np.uint64).tolist()
        else:
            out[c] = [None if x is None or x is np.nan or (isinstance(x, float) and x != x)
                      else x for x in col.tolist()]
    return out
