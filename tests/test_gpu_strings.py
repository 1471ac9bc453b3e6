"""String columns of a scan unit decoded on the GPU (csrc/hip/strings.hip):
the two kernels on synthetic tensors, the production decoder
(read_unit_raw(gpu_strings=True) -> UnitTransfer -> hip().decode_unit) on
pyarrow and project files, and whole scans with LAKESOUL_GPU_STRINGS=1 / 0
in fresh child processes. Every comparison is byte-exact against the Python
lists the inputs were built from. Without the feature the tests fail at
gpu_strings=True, UD_STR and the missing bindings."""

import json
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import encoding_cases as ec
import string_cases as sc

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests require an MI355X"
    return torch.device("cuda:0")


# ---- strip_prefixes, direct ------------------------------------------- #

def _strip_guarded(dev, vals, shift):
    """strip_prefixes into a slice that starts `shift` bytes into a buffer
    of guard bytes: the slice equals the values, the guards are unchanged."""
    from lakesoul_amd.ops import hip

    raw, offs = sc.plain_stream(vals)
    want = b"".join(vals)
    buf = torch.full((GUARD + len(want) + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    lo = GUARD - 8 + shift
    out = buf[lo:lo + len(want)]
    got = hip().strip_prefixes(torch.from_numpy(raw).to(dev),
                               torch.from_numpy(offs).to(dev), out=out)
    assert got.data_ptr() == out.data_ptr()
    host = buf.cpu().numpy()
    assert host[lo:lo + len(want)].tobytes() == want
    assert (host[:lo] == 0xA5).all() and (host[lo + len(want):] == 0xA5).all()


@pytest.mark.parametrize("name", list(sc.strip_cases()))
def test_strip_prefixes_direct(dev, name):
    from lakesoul_amd.ops import hip

    vals = sc.strip_cases()[name]
    for shift in (0, 3, 7):  # the destination at three word phases
        _strip_guarded(dev, vals, shift)
    raw, offs = sc.plain_stream(vals)
    got = hip().strip_prefixes(torch.from_numpy(raw).to(dev),
                               torch.from_numpy(offs).to(dev))
    assert got.cpu().numpy().tobytes() == b"".join(vals)


def test_strip_prefixes_grid_stride(dev):
    """About 12 MB: more tiles than the 2048 workgroups of the grid."""
    vals = sc.stride_case()
    assert sum(map(len, vals)) > 2048 * sc.TILE
    _strip_guarded(dev, vals, 5)


# ---- dict_strings, direct --------------------------------------------- #

@pytest.mark.parametrize("kind", sc.VALIDITY_KINDS)
@pytest.mark.parametrize("nent", sc.DICT_SIZES)
def test_dict_strings_direct(dev, nent, kind):
    from lakesoul_amd.ops import hip

    _, doff, dby = sc.dictionary(nent)
    idx, v, want = sc.dict_rows(nent, 3000, kind)
    offs, by, status = hip().dict_strings(
        torch.from_numpy(idx).to(dev), torch.from_numpy(doff).to(dev),
        torch.from_numpy(dby).to(dev),
        None if v is None else torch.from_numpy(v).to(dev))
    assert int(status[0]) == 0
    assert sc.rows_of(offs.cpu().numpy(), by.cpu().numpy(), v) == want


def test_dict_strings_bad_index(dev):
    """idx holding the dictionary size and INT32_MAX: the status is set,
    those rows are empty, the others right. The kernel's bounds check on
    valid memory."""
    from lakesoul_amd.ops import hip

    nent = 300
    _, doff, dby = sc.dictionary(nent)
    idx, v, want = sc.dict_rows(nent, 3000, "some")
    idx[3], idx[1500] = nent, np.iinfo(np.int32).max
    rows = np.flatnonzero(v)
    want[rows[3]] = want[rows[1500]] = b""
    offs, by, status = hip().dict_strings(
        torch.from_numpy(idx).to(dev), torch.from_numpy(doff).to(dev),
        torch.from_numpy(dby).to(dev), torch.from_numpy(v).to(dev))
    assert int(status[0]) != 0
    assert sc.rows_of(offs.cpu().numpy(), by.cpu().numpy(), v) == want


# ---- through the production decoder ------------------------------------ #

def _bufs(dev, raw):
    from lakesoul_amd.io.reader_gpu import UnitTransfer

    tr = UnitTransfer(raw, dev)
    e_u8 = torch.empty(0, dtype=torch.uint8, device=dev)
    e_i64 = torch.empty(0, dtype=torch.int64, device=dev)
    return (tr.vals, tr.validity if tr.validity is not None else e_u8,
            tr.dicts if tr.dicts is not None else e_u8,
            tr.runs if tr.runs is not None else e_i64,
            tr.soffs if tr.soffs is not None else e_i64, raw["desc"]), tr.enc


def _decode(dev, raw, nfiles, ncols):
    from lakesoul_amd.ops import hip

    bufs, enc = _bufs(dev, raw)
    return hip().decode_unit(*bufs, nfiles, ncols, enc)


def _entry_rows(entry):
    offs, by, valid = entry
    v = None if valid is None else valid.cpu().numpy()
    return sc.rows_of(offs.cpu().numpy(), by.cpu().numpy(), v)


def _same_entry(a, b, what):
    """Two decoded string entries, bit for bit."""
    assert torch.equal(a[0], b[0]), what
    assert torch.equal(a[1], b[1]), what
    assert (a[2] is None) == (b[2] is None), what
    if a[2] is not None:
        assert torch.equal(a[2], b[2]), what


def _check_unit(dev, path, cols, tags):
    """cols: name -> (list of str, mask); an int32 column `p` sits in front.
    The tags are asserted, so nothing passes by falling back; the decoded
    triple equals the host route's bit for bit, and the inputs."""
    from lakesoul_amd.ops import cpp

    names = ["p"] + list(cols)
    raw = sc.read_unit_strings([path], names)
    desc = raw["desc"].numpy()
    assert desc[0, cpp().UD_STR] == 0
    for u, name in enumerate(names[1:], 1):
        want_tag = tags[name]
        got_tag = int(desc[u, cpp().UD_STR])
        assert got_tag in want_tag if isinstance(want_tag, tuple) \
            else got_tag == want_tag, (name, got_tag)
        assert got_tag != 0 and desc[u, cpp().UD_VAL_OFF] > 0, name
    outs = _decode(dev, raw, 1, len(names))
    host = _decode(dev, sc.read_unit_strings([path], names, gpu_strings=False),
                   1, len(names))
    n = len(next(iter(cols.values()))[0])
    np.testing.assert_array_equal(
        outs[0][0].view(torch.int32).cpu().numpy(), np.arange(n, dtype=np.int32))
    for u, name in enumerate(names[1:], 1):
        vals, mask = cols[name]
        assert _entry_rows(outs[u]) == sc.expected(vals, mask), name
        _same_entry(outs[u], host[u], name)


@pytest.mark.parametrize("codec", ec.CODECS)
@pytest.mark.parametrize("version", ec.VERSIONS)
@pytest.mark.parametrize("encoding", sc.STRING_ENCODINGS)
def test_pyarrow_files_gpu(dev, tmp_path, encoding, version, codec):
    tag = sc.expected_tag(encoding)
    for name, vals in ec.string_sets().items():
        n = len(vals)
        cols = {"s": (vals, None), "sn": (vals, ec.null_mask(n, "some", n))}
        path = sc.write_strings(tmp_path / f"{name}.parquet", cols, encoding,
                                version, codec)
        _check_unit(dev, path, cols, {"s": tag, "sn": tag})


@pytest.mark.parametrize("encoding", sc.STRING_ENCODINGS)
def test_multi_page_multi_chunk_gpu(dev, tmp_path, encoding):
    """Several pages per chunk, three chunks, a whole row group null, an
    all-null column."""
    from lakesoul_amd.ops import cpp

    cols = sc.multi_string_columns()
    path = sc.write_strings(tmp_path / "multi.parquet", cols, encoding, "2.0",
                            "zstd", **ec.MULTI_KW)
    tag = sc.expected_tag(encoding)
    _check_unit(dev, path, cols, {"keys": tag, "low": tag,
                                  "allnull": (cpp().UD_STR_PLAIN, cpp().UD_STR_DICT)})


def test_project_file_gpu(dev, tmp_path):
    from lakesoul_amd.ops import cpp

    vals = ec.string_sets()["unicode"] * 9
    mask = ec.null_mask(len(vals), "some", 4)
    path = sc.write_project_file(tmp_path / "ours.parquet", vals, mask)
    _check_unit(dev, path, {"s": (vals, None), "sn": (vals, mask)},
                {"s": cpp().UD_STR_PLAIN, "sn": cpp().UD_STR_PLAIN})


def test_three_file_unit_gpu(dev, tmp_path):
    """PLAIN in one file, dictionary in the next, absent in the third."""
    from lakesoul_amd.ops import cpp

    a = ec.string_sets()["prefix"]
    b = [["AIR", "R", "TRUCK"][i % 3] for i in range(200)]
    files = [
        sc.write_strings(tmp_path / "plain.parquet", {"x": (a, None)}, "PLAIN"),
        sc.write_strings(tmp_path / "dict.parquet", {"x": (b, None)}, "RLE_DICTIONARY"),
        sc.write_strings(tmp_path / "none.parquet", {"y": (a, None)}, "PLAIN"),
    ]
    raw = sc.read_unit_strings(files, ["x"])
    assert raw["desc"][:, cpp().UD_STR].tolist() == [
        cpp().UD_STR_PLAIN, cpp().UD_STR_DICT, 0]
    outs = _decode(dev, raw, 3, 1)
    host = _decode(dev, sc.read_unit_strings(files, ["x"], gpu_strings=False), 3, 1)
    assert _entry_rows(outs[0]) == [x.encode() for x in a]
    assert _entry_rows(outs[1]) == [x.encode() for x in b]
    assert outs[2] is None and host[2] is None
    _same_entry(outs[0], host[0], "plain")
    _same_entry(outs[1], host[1], "dict")


def test_one_total_readback_per_unit(dev, tmp_path):
    """Two files x two dictionary string columns through scan_unit_uselast:
    the byte totals of all four come back in ONE copy."""
    from lakesoul_amd.ops import cpp, hip

    low = ["AIR", "R", "TRUCK", "", "REG AIR", "MAIL", "SHIP-LONGER"]
    files, want = [], {}
    for f in range(2):
        ids = np.arange(f * 500, f * 500 + 1000, dtype=np.int64)
        a = [low[(int(i) + f) % 7] for i in ids]
        b = [f"b{f}-{int(i) % 13}" for i in ids]
        mask = ec.null_mask(len(ids), "some", f)
        path = str(tmp_path / f"f{f}.parquet")
        pq.write_table(pa.table({"id": pa.array(ids), "a": pa.array(a),
                                 "b": pa.array(b, mask=mask)}), path,
                       use_dictionary=["a", "b"], compression="zstd")
        files.append(path)
        for i, x, y, m in zip(ids.tolist(), a, b, mask.tolist()):
            want[i] = (x.encode(), None if m else y.encode())
    raw = sc.read_unit_strings(files, ["id", "a", "b"])
    assert raw["desc"][:, cpp().UD_STR].tolist() == [0, 2, 2, 0, 2, 2]
    bufs, enc = _bufs(dev, raw)
    before = hip().dict_total_readbacks()
    outs = hip().scan_unit_uselast(*bufs, 2, 3, 0, 8, enc)
    assert hip().dict_total_readbacks() - before == 1
    ids = outs[0][0].view(torch.int64).cpu().tolist()
    assert ids == sorted(want)
    got = dict(zip(ids, zip(_entry_rows(outs[1]), _entry_rows(outs[2]))))
    assert got == want


# ---- scans, in fresh child processes ----------------------------------- #

def _foreign_dict_file(path, columns):
    """A pyarrow file whose string columns are all dictionary-encoded."""
    tbl = pa.table(columns)
    strs = [n for n in tbl.column_names if pa.types.is_string(tbl.schema.field(n).type)]
    pq.write_table(tbl, str(path), use_dictionary=strs, compression="zstd",
                   data_page_size=2048, write_batch_size=128)
    md = pq.ParquetFile(str(path)).metadata
    for i, n in enumerate(tbl.column_names):
        if n in strs:
            assert md.row_group(0).column(i).has_dictionary_page, n
    return str(path)


def _build_tables(root):
    """Five tables in one catalog, each with files of ours (PLAIN strings)
    and committed foreign files with dictionary-encoded string columns."""
    from lakesoul_amd.io.schema import Field, Schema

    catalog = ec.mk_catalog(root)
    names = []
    # the foreign table of the encodings tests, `s` also dictionary-encoded:
    # single int64 PK (one-call unit path) and two PKs (generic path)
    for name, pks in (("str_fast", ["id"]), ("str_generic", ["id", "id2"])):
        sub = root / name
        sub.mkdir()
        t, _, _ = ec.foreign_table(sub, catalog, pks, name=name)
        fid = np.arange(500, 3200, 3, dtype=np.int64)
        k = len(fid)
        ec.commit_foreign(t, _foreign_dict_file(
            sub / "part-foreigndict000_0000.parquet",
            {"id": pa.array(fid), "id2": pa.array((fid % 5).astype(np.int32)),
             "c": pa.array(fid * 3), "v": pa.array(fid.astype(np.float64)),
             "s": pa.array([f"dict-value-{i % 7}" * (i % 3) for i in range(k)],
                           type=pa.string(), mask=ec.null_mask(k, "some", 5))}))
        names.append(name)
    # string primary key
    sub = root / "str_pk"
    sub.mkdir()
    t = catalog.create_table(
        "str_pk", Schema([Field("k", "string", False), Field("v", "int64")]),
        primary_keys=["k"], hash_bucket_num=1)
    keys = [f"org/unit/key-{i:06d}" for i in range(1000)]
    t.upsert({"k": keys, "v": np.zeros(1000, dtype=np.int64)}, device="cpu")
    fkeys = keys[:300:2] + [f"org/unit/new-{i:06d}" for i in range(50)]
    ec.commit_foreign(t, _foreign_dict_file(
        sub / "part-foreigndict000_0000.parquet",
        {"k": pa.array(fkeys, type=pa.string()),
         "v": pa.array(np.arange(1, len(fkeys) + 1, dtype=np.int64))}))
    names.append("str_pk")
    # JoinedAllByComma on a dictionary column
    sub = root / "str_join"
    sub.mkdir()
    t = catalog.create_table(
        "str_join", Schema([Field("id", "int64", False), Field("tags", "string")]),
        primary_keys=["id"], hash_bucket_num=1,
        properties={"merge_op.tags": "JoinedAllByComma"})
    n = 2000
    t.upsert({"id": np.arange(n, dtype=np.int64),
              "tags": [f"a{i % 11}" for i in range(n)]}, device="cpu")
    fid = np.arange(0, n, 3, dtype=np.int64)
    ec.commit_foreign(t, _foreign_dict_file(
        sub / "part-foreigndict000_0000.parquet",
        {"id": pa.array(fid),
         "tags": pa.array([["x", "yy", "", "zzz"][i % 4] for i in range(len(fid))],
                          type=pa.string(), mask=ec.null_mask(len(fid), "some", 9))}))
    names.append("str_join")
    # CDC with a dictionary-encoded rowKinds column
    sub = root / "str_cdc"
    sub.mkdir()
    t = catalog.create_table(
        "str_cdc", Schema([Field("id", "int64", False), Field("v", "float64"),
                           Field("rowKinds", "string")]),
        primary_keys=["id"], hash_bucket_num=1,
        properties={"lakesoul_cdc_change_column": "rowKinds"})
    n = 1000
    t.upsert({"id": np.arange(n, dtype=np.int64), "v": np.ones(n),
              "rowKinds": ["insert"] * n}, device="cpu")
    fid = np.arange(0, n, 4, dtype=np.int64)
    ec.commit_foreign(t, _foreign_dict_file(
        sub / "part-foreigndict000_0000.parquet",
        {"id": pa.array(fid), "v": pa.array(np.zeros(len(fid))),
         "rowKinds": pa.array([["delete", "update", "insert"][i % 3]
                               for i in range(len(fid))], type=pa.string())}))
    names.append("str_cdc")
    return catalog, names


def _run_child(root, names, flag):
    out = root / f"child{flag}"
    out.mkdir()
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                         "gpu_strings_child.py")
    env = dict(os.environ, LAKESOUL_GPU_STRINGS=flag)
    r = subprocess.run(
        [sys.executable, child, str(out), str(root / "meta.db"), str(root / "wh"),
         ",".join(names)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    scans = {n: pa.ipc.open_file(str(out / f"{n}.arrow")).read_all() for n in names}
    return scans, json.load(open(out / "tags.json"))


@pytest.fixture(scope="module")
def scans(dev, tmp_path_factory):
    """Every table scanned on the GPU with the route on and off, each in
    one fresh process, and on the CPU here."""
    root = tmp_path_factory.mktemp("string_scans")
    catalog, names = _build_tables(root)
    on, tags_on = _run_child(root, names, "1")
    off, tags_off = _run_child(root, names, "0")
    cpu = {n: catalog.table(n).scan(device="cpu").to_arrow() for n in names}
    return on, off, cpu, tags_on, tags_off


@pytest.mark.parametrize("name,key", [
    ("str_fast", "id"), ("str_generic", "id"), ("str_pk", "k"),
    ("str_join", "id"), ("str_cdc", "id")])
def test_scan_same_with_route_on_off_and_cpu(scans, name, key):
    on, off, cpu, tags_on, tags_off = scans
    a = on[name].sort_by(key)
    assert a.num_rows > 0
    cols = [c for c in a.column_names if not pa.types.is_floating(a.schema.field(c).type)]
    assert cols
    for other in (off[name], cpu[name]):
        b = other.sort_by(key).select(a.column_names)
        assert a.num_rows == b.num_rows
        for c in a.column_names:
            x, y = a.column(c).to_pylist(), b.column(c).to_pylist()
            if c in cols:
                assert x == y, (name, c)
            else:  # NaNs: compare bit patterns
                xb = np.array([np.nan if v is None else v for v in x]).view(np.uint64)
                yb = np.array([np.nan if v is None else v for v in y]).view(np.uint64)
                np.testing.assert_array_equal(xb, yb, err_msg=f"{name}.{c}")
                assert [v is None for v in x] == [v is None for v in y]
    flat_on = [t for unit in tags_on[name] for t in unit]
    flat_off = [t for unit in tags_off[name] for t in unit]
    assert 1 in flat_on and 2 in flat_on, flat_on
    assert flat_off and not any(flat_off), flat_off


def test_scan_contents(scans):
    """The merged tables hold what the dictionary files brought."""
    on = scans[0]
    s = on["str_fast"].sort_by("id").column("s").to_pylist()
    assert "dict-value-1" in s and "dict-value-2dict-value-2" in s and "ours" in s
    tags = on["str_join"].sort_by("id").column("tags").to_pylist()
    assert any(t is not None and "," in t for t in tags)
    ids = set(on["str_cdc"].column("id").to_pylist())
    assert 0 not in ids and 4 in ids and 1 in ids
