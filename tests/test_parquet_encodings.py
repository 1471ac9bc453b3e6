"""Foreign parquet files in the "v2" value encodings — DELTA_BINARY_PACKED,
BYTE_STREAM_SPLIT, DELTA_LENGTH_BYTE_ARRAY, DELTA_BYTE_ARRAY — through the
host decoders (csrc/cpp/delta.h): read_chunk_cpu, read_unit_raw with the
host route, and a table scan(device="cpu") of a foreign file next to an
upsert of ours. pyarrow writes every file (dictionary off, column_encoding
set); expected values are the numpy inputs, cross-checked against
pq.read_table. Every comparison is bit-exact (floats through an integer
view).

Before these encodings were read, every case here ended in
`unsupported data encoding N` from ParquetFile::read_chunk_impl: that is
how the tests fail without the feature. No GPU is needed; the GPU kernels
are covered by test_gpu_encodings.py."""

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import encoding_cases as ec

MATRIX = [(v, c, o) for v in ec.VERSIONS for c in ec.CODECS
          for o in (False, True)]
MATRIX_IDS = [f"v{v[0]}-{c}-{'optional' if o else 'required'}"
              for v, c, o in MATRIX]


def _arrays(values, optional, seed, null_kind="some", types=None):
    """name -> (numpy values, null mask or None, pyarrow array)"""
    out = {}
    for k, (name, v) in enumerate(values.items()):
        mask = ec.null_mask(len(v), null_kind, seed + k) if optional else None
        typ = (types or {}).get(name)
        out[name] = (v, mask, pa.array(v, type=typ, mask=mask))
    return out


def _check_fixed(path, cols, np_phys=None):
    """Every column of `path` through read_chunk_cpu, the host-route unit
    and pq.read_table against the numpy input."""
    names = list(cols)
    raw = ec.read_unit_host([path], names)
    ref = pq.read_table(path)
    for ci, name in enumerate(names):
        v, mask, _ = cols[name]
        valid = np.ones(len(v), bool) if mask is None else ~mask
        phys = np_phys or v.dtype
        want = ec.bits(v.astype(phys))
        got, gvalid = ec.read_chunks_cpu(path, ci, want.dtype)
        np.testing.assert_array_equal(gvalid, valid, err_msg=name)
        np.testing.assert_array_equal(got[valid], want[valid], err_msg=name)
        dense, uvalid = ec.unit_plain_column(raw, ci, want.dtype)
        np.testing.assert_array_equal(uvalid, valid, err_msg=name)
        np.testing.assert_array_equal(dense, want[valid], err_msg=name)
        # pyarrow's own reader agrees with the input
        rcol = ref.column(name)
        assert rcol.null_count == int((~valid).sum()), name
        if np_phys is None:
            rv = rcol.combine_chunks().drop_null().to_numpy()
            np.testing.assert_array_equal(ec.bits(rv), want[valid], err_msg=name)


@pytest.mark.parametrize("version,codec,optional", MATRIX, ids=MATRIX_IDS)
def test_delta_binary_packed(tmp_path, version, codec, optional):
    """INT64 (256/4 blocks) and INT32 (128/4) at every boundary row count:
    tiny widths, width 0, growing widths, a width-64 / width-32 miniblock,
    wraparound, and the full range."""
    for np_dtype, counts in ((np.int64, ec.INT64_COUNTS),
                             (np.int32, ec.INT32_COUNTS)):
        for n in counts:
            cols = _arrays(ec.int_value_sets(np_dtype, n, seed=n), optional, n)
            path = ec.write(
                tmp_path / f"dbp_{np.dtype(np_dtype).name}_{n}.parquet",
                {k: a for k, (_, _, a) in cols.items()},
                {k: "DELTA_BINARY_PACKED" for k in cols}, version, codec)
            _check_fixed(path, cols)


@pytest.mark.parametrize("version", ec.VERSIONS)
@pytest.mark.parametrize("optional", [False, True], ids=["required", "optional"])
def test_delta_binary_packed_logical_types(tmp_path, version, optional):
    """int8 / int16 / date32 (physical INT32) and timestamp[us] /
    decimal(18,2) (physical INT64) columns."""
    n = 130
    rng = np.random.default_rng(5)
    i32 = {
        "i8": (rng.integers(-128, 127, n, endpoint=True).astype(np.int8), pa.int8()),
        "i16": (rng.integers(-2**15, 2**15 - 1, n, endpoint=True).astype(np.int16), pa.int16()),
        "d32": (rng.integers(-10**6, 10**6, n).astype(np.int32), pa.date32()),
    }
    i64 = {
        "ts": (np.sort(rng.integers(0, 2**52, n)).astype(np.int64), pa.timestamp("us")),
    }
    for group, phys in ((i32, np.int32), (i64, np.int64)):
        cols = _arrays({k: v for k, (v, _) in group.items()}, optional, 3,
                       types={k: t for k, (_, t) in group.items()})
        path = ec.write(tmp_path / f"logical_{np.dtype(phys).name}.parquet",
                        {k: a for k, (_, _, a) in cols.items()},
                        {k: "DELTA_BINARY_PACKED" for k in cols}, version)
        _check_fixed(path, cols, np_phys=phys)
    # decimal(18,2): unscaled int64 when the writer stores it as an integer
    import decimal

    unscaled = rng.integers(-10**17, 10**17, n).astype(np.int64)
    mask = ec.null_mask(n, "some", 9) if optional else None
    dec = pa.array([decimal.Decimal(int(x)).scaleb(-2) for x in unscaled],
                   type=pa.decimal128(18, 2), mask=mask)
    path = str(tmp_path / "dec.parquet")
    pq.write_table(pa.table({"d": dec}), path, use_dictionary=False,
                   column_encoding={"d": "DELTA_BINARY_PACKED"},
                   store_decimal_as_integer=True, data_page_version=version)
    md = pq.ParquetFile(path).metadata.row_group(0).column(0)
    assert md.physical_type == "INT64" and "DELTA_BINARY_PACKED" in md.encodings
    _check_fixed(path, {"d": (unscaled, mask, dec)}, np_phys=np.int64)


@pytest.mark.parametrize("version,codec,optional", MATRIX, ids=MATRIX_IDS)
def test_byte_stream_split(tmp_path, version, codec, optional):
    """FLOAT, DOUBLE, INT32, INT64 at 1, 63, 64, 65 values: NaNs with
    payload bits, both zeros, both infinities, full-range integers."""
    for n in ec.BSS_COUNTS:
        values = {
            "f32": ec.float_specials(np.float32, n, n),
            "f64": ec.float_specials(np.float64, n, n + 1),
            "i32": ec.int_value_sets(np.int32, n, n)["random"],
            "i64": ec.int_value_sets(np.int64, n, n)["random"],
        }
        cols = _arrays(values, optional, n)
        path = ec.write(tmp_path / f"bss_{n}.parquet",
                        {k: a for k, (_, _, a) in cols.items()},
                        {k: "BYTE_STREAM_SPLIT" for k in cols}, version, codec)
        _check_fixed(path, cols)


@pytest.mark.parametrize("version", ec.VERSIONS)
@pytest.mark.parametrize("codec", ec.CODECS)
@pytest.mark.parametrize("null_kind", [None, "page"], ids=["required", "nulls"])
def test_multi_page_multi_chunk(tmp_path, version, codec, null_kind):
    """5000 rows in small pages and three row groups; with nulls: ~30 %,
    a row group whose pages are entirely null, and a column that is
    entirely null. The unit's own page table (the rows read_unit_raw lists
    for the GPU decoders) must show more pages than chunks, and the file
    more than one chunk, so the case cannot shrink to a single page."""
    from lakesoul_amd.ops import cpp

    plain, encs = ec.multi_columns(null_kind)
    cols = {k: (v, m, pa.array(v, mask=m)) for k, (v, m) in plain.items()}
    path = ec.write(tmp_path / "multi.parquet",
                    {k: a for k, (_, _, a) in cols.items()}, encs, version,
                    codec, **ec.MULTI_KW)
    nchunks = pq.ParquetFile(path).metadata.num_row_groups
    assert nchunks > 1
    raw = ec.read_unit_gpu_route([path], list(cols))
    desc = raw["desc"].numpy()
    for u, name in enumerate(cols):
        assert desc[u, cpp().UD_ENC] == (1 if encs[name].startswith("DELTA") else 2), name
        # the full-range columns fill a 512-byte page every 64 values;
        # the sorted and the constant / all-null ones pack far smaller
        if name in ("a", "b", "f", "g"):
            assert desc[u, cpp().UD_ENC_PAGES] > 2 * nchunks, (name, desc[u])
        else:
            assert desc[u, cpp().UD_ENC_PAGES] >= nchunks, (name, desc[u])
    _check_fixed(path, cols)


def _string_arrays(optional):
    out = {}
    for k, (name, vals) in enumerate(ec.string_sets().items()):
        mask = ec.null_mask(len(vals), "some", k) if optional else None
        out[name] = (vals, mask)
    return out


@pytest.mark.parametrize("version,codec,optional", MATRIX, ids=MATRIX_IDS)
@pytest.mark.parametrize("enc", ["DELTA_LENGTH_BYTE_ARRAY", "DELTA_BYTE_ARRAY"])
def test_delta_strings(tmp_path, enc, version, codec, optional):
    """Empty strings, one 5000-byte value, sorted keys with long shared
    prefixes, non-ASCII text (compared as bytes), nulls; the long sets in
    small pages and several row groups."""
    for name, (vals, mask) in _string_arrays(optional).items():
        arr = pa.array(vals, type=pa.string(), mask=mask)
        kw = dict(data_page_size=512, write_batch_size=32, row_group_size=120) \
            if len(vals) > 100 else {}
        path = ec.write(tmp_path / f"s_{name}.parquet", {"s": arr}, {"s": enc},
                        version, codec, **kw)
        if kw:
            assert pq.ParquetFile(path).metadata.num_row_groups > 1
        want = [None if mask is not None and mask[i] else v.encode()
                for i, v in enumerate(vals)]
        assert ec.read_chunks_cpu_strings(path, 0) == want, name
        assert ec.unit_string_column(ec.read_unit_host([path], ["s"]), 0) == want, name
        ref = pq.read_table(path).column("s").to_pylist()
        assert [None if r is None else r.encode() for r in ref] == want, name


@pytest.mark.parametrize("pks", [["id"], ["id", "id2"]], ids=["single_pk", "composite_pk"])
def test_table_scan_cpu_foreign_encodings(tmp_path, catalog, pks):
    t, exp, (fid, fc, cmask) = ec.foreign_table(tmp_path, catalog, pks)
    got = t.scan(device="cpu").to_arrow()
    # exact integer check of the nullable DBP column, nulls included
    got = got.sort_by("id")
    gc = got.column("c").to_pylist()
    by_id = dict(zip(got.column("id").to_pylist(), gc))
    for i, x, isnull in zip(fid.tolist(), fc.tolist(), cmask.tolist()):
        assert by_id[i] == (None if isnull else x), i
    df = got.to_pandas()
    assert len(df) == len(exp)
    assert ec.frame_bits(df[["id", "id2", "v", "s"]]) == ec.frame_bits(exp[["id", "id2", "v", "s"]])


def test_table_scan_cpu_string_pk_foreign(tmp_path, catalog):
    """A string PRIMARY KEY column of a foreign file in DELTA_BYTE_ARRAY
    (and once DELTA_LENGTH_BYTE_ARRAY) merged with an upsert of ours."""
    from lakesoul_amd.io.schema import Field, Schema

    for enc in ("DELTA_BYTE_ARRAY", "DELTA_LENGTH_BYTE_ARRAY"):
        t = catalog.create_table(
            "spk_" + enc.lower(),
            Schema([Field("k", "string", False), Field("v", "int64")]),
            primary_keys=["k"], hash_bucket_num=1)
        n, m = 1000, 300
        keys = [f"org/unit/key-{i:06d}" for i in range(n)]
        t.upsert({"k": keys, "v": np.zeros(n, dtype=np.int64)}, device="cpu")
        fkeys = keys[:m] + [f"org/unit/new-{i:06d}" for i in range(50)]
        fv = np.arange(1, len(fkeys) + 1, dtype=np.int64)
        (tmp_path / enc).mkdir()
        foreign = ec.write(
            tmp_path / enc / "part-foreign0000000_0000.parquet",
            {"k": pa.array(fkeys, type=pa.string()), "v": pa.array(fv)},
            {"k": enc, "v": "DELTA_BINARY_PACKED"}, "1.0", "snappy",
            data_page_size=1024, write_batch_size=64)
        ec.commit_foreign(t, foreign)
        got = t.scan(device="cpu").to_arrow().sort_by("k")
        want = {k: 0 for k in keys}
        want.update(dict(zip(fkeys, fv.tolist())))
        assert got.column("k").to_pylist() == sorted(want)
        assert got.column("v").to_pylist() == [want[k] for k in sorted(want)]


from test_capi_v2 import _cfg_reader, _read_all, _write_sorted_file, lib  # noqa: E402,F401


def test_c_engine_reads_foreign_encodings(lib, tmp_path):  # noqa: F811
    """The C ABI reader merges a file of ours with a foreign file whose
    key is DELTA_BINARY_PACKED, value BYTE_STREAM_SPLIT and string
    DELTA_BYTE_ARRAY."""
    import ctypes

    from lakesoul_amd.io.schema import Field, Schema

    schema = Schema([Field("id", "int64", False), Field("v", "float64"),
                     Field("s", "string")])
    ours = str(tmp_path / "base.parquet")
    _write_sorted_file(ours, {"id": np.arange(300, dtype=np.int64),
                              "v": np.full(300, 1.0),
                              "s": [f"a{i}" for i in range(300)]}, schema)
    fid = np.arange(0, 400, 2, dtype=np.int64)
    fv = np.random.default_rng(4).normal(size=len(fid))
    foreign = ec.write(
        tmp_path / "foreign.parquet",
        {"id": pa.array(fid), "v": pa.array(fv),
         "s": pa.array([f"prefix/shared/{i:05d}" for i in fid], type=pa.string())},
        {"id": "DELTA_BINARY_PACKED", "v": "BYTE_STREAM_SPLIT",
         "s": "DELTA_BYTE_ARRAY"}, "2.0", "zstd")
    r = _cfg_reader(lib, [ours, foreign], pks=["id"])
    df = _read_all(lib, r).sort_values("id").reset_index(drop=True)
    lib.lakesoul_c_reader_close(ctypes.c_void_p(r))
    want_v = {i: 1.0 for i in range(300)}
    want_v.update(dict(zip(fid.tolist(), fv.tolist())))
    want_s = {i: f"a{i}" for i in range(300)}
    want_s.update({int(i): f"prefix/shared/{i:05d}" for i in fid})
    assert df["id"].tolist() == sorted(want_v)
    assert ec.bits(df["v"].to_numpy()).tolist() == \
        ec.bits(np.array([want_v[i] for i in sorted(want_v)])).tolist()
    assert df["s"].tolist() == [want_s[i] for i in sorted(want_s)]


def test_mixed_files_in_one_unit(tmp_path):
    """One unit, same column: a PLAIN file, a DELTA_BINARY_PACKED file and
    a file that lacks the column. Host route: three plain columns. GPU
    route: only the delta file's column is listed for the GPU decoder."""
    from lakesoul_amd.ops import cpp

    n = 300
    a = ec.int_value_sets(np.int64, n, 1)["random"]
    b = ec.int_value_sets(np.int64, n, 2)["random"]
    p_plain = ec.write(tmp_path / "plain.parquet", {"x": pa.array(a)}, {"x": "PLAIN"})
    p_delta = ec.write(tmp_path / "delta.parquet", {"x": pa.array(b)},
                       {"x": "DELTA_BINARY_PACKED"})
    p_none = ec.write(tmp_path / "none.parquet", {"y": pa.array(a)}, {"y": "PLAIN"})
    files = [p_plain, p_delta, p_none]
    raw = ec.read_unit_host(files, ["x"])
    desc = raw["desc"].numpy()
    assert desc[:, cpp().UD_PRESENT].tolist() == [1, 1, 0]
    assert raw["enc"].numel() == 0 and not desc[:, cpp().UD_ENC].any()
    np.testing.assert_array_equal(ec.unit_plain_column(raw, 0, np.int64)[0], a)
    np.testing.assert_array_equal(ec.unit_plain_column(raw, 1, np.int64)[0], b)
    raw = ec.read_unit_gpu_route(files, ["x"])
    desc = raw["desc"].numpy()
    assert desc[:, cpp().UD_PRESENT].tolist() == [1, 1, 0]
    assert desc[:, cpp().UD_ENC].tolist() == [0, cpp().UD_ENC_DELTA_BINARY, 0]
    np.testing.assert_array_equal(ec.unit_plain_column(raw, 0, np.int64)[0], a)


@pytest.mark.parametrize("codec", ["none", "zstd"])
def test_dictionary_chunk_with_fallback_pages(tmp_path, codec):
    """A dictionary chunk whose later pages fall back to another encoding
    is a plain chunk to everything downstream, and a column that mixes it
    with a dictionary-only row group is a plain column of the unit."""
    from lakesoul_amd.ops import cpp

    path, a, s = ec.write_dict_fallback(tmp_path / "fallback.parquet", codec)
    h = cpp().open_parquet(path)
    try:
        kinds = [[bool(cpp().read_chunk_raw(h, rg, c)["is_dict"]) for rg in range(2)]
                 for c in range(2)]
    finally:
        cpp().close_parquet(h)
    # row group 0 keeps its dictionary; row group 1 fell back and is plain
    assert kinds == [[True, False], [True, False]]
    got, valid = ec.read_chunks_cpu(path, 0, np.int64)
    assert valid.all()
    np.testing.assert_array_equal(got, a)
    want_s = [x.encode() for x in s]
    assert ec.read_chunks_cpu_strings(path, 1) == want_s
    for raw in (ec.read_unit_host([path], ["a", "s"]),
                ec.read_unit_gpu_route([path], ["a", "s"])):
        dense, _ = ec.unit_plain_column(raw, 0, np.int64)
        np.testing.assert_array_equal(dense, a)
        assert raw["runs"].numel() == 0  # no dictionary lane left
        assert ec.unit_string_column(raw, 1) == want_s


def test_out_of_scope_encodings_stay_errors(tmp_path):
    """BYTE_STREAM_SPLIT / DELTA_BYTE_ARRAY on FIXED_LEN_BYTE_ARRAY keep a
    clear error."""
    from lakesoul_amd.ops import cpp

    arr = pa.array([b"abcd", b"efgh", b"ijkl"], type=pa.binary(4))
    for enc in ("BYTE_STREAM_SPLIT", "DELTA_BYTE_ARRAY"):
        path = ec.write(tmp_path / f"flba_{enc}.parquet", {"x": arr}, {"x": enc})
        h = cpp().open_parquet(path)
        try:
            with pytest.raises(RuntimeError, match="unsupported data encoding"):
                cpp().read_chunk_cpu(h, 0, 0)
        finally:
            cpp().close_parquet(h)


def test_delta_sanitizer_clean(tmp_path):
    """The delta.h walk and decoders under AddressSanitizer + UBSan
    (csrc/cpp/tests/delta_san.cc, a stand-alone program): round-trips of
    the value sets above in the 128/4 and 256/4 layouts, then every
    truncation and single-byte change of each stream. Any return or throw
    is fine, a sanitizer report is not, and every miniblock the walk
    reports must lie inside the buffer — what the GPU kernel relies on."""
    import os
    import shutil
    import subprocess

    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "csrc", "cpp", "tests", "delta_san.cc")
    exe = str(tmp_path / "delta_san")
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
