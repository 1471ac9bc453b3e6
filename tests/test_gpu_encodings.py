"""DELTA_BINARY_PACKED and BYTE_STREAM_SPLIT pages decoded on the GPU
(csrc/hip/delta.hip), and the two string encodings through the GPU scan.
The decoder checks go through the production decoder: read_unit_raw (GPU
route) -> UnitTransfer -> hip().decode_unit, on the files of the CPU matrix
(encoding_cases.py). Every comparison is bit-exact. Without the feature
every file here ends in `unsupported data encoding N`."""

import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pytest
import torch

import encoding_cases as ec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests require an MI355X"
    return torch.device("cuda:0")


def _decode(dev, raw, nfiles, ncols):
    from lakesoul_amd.io.reader_gpu import UnitTransfer
    from lakesoul_amd.ops import hip

    tr = UnitTransfer(raw, dev)
    e_u8 = torch.empty(0, dtype=torch.uint8, device=dev)
    e_i64 = torch.empty(0, dtype=torch.int64, device=dev)
    return hip().decode_unit(
        tr.vals, tr.validity if tr.validity is not None else e_u8,
        tr.dicts if tr.dicts is not None else e_u8,
        tr.runs if tr.runs is not None else e_i64,
        tr.soffs if tr.soffs is not None else e_i64, raw["desc"], nfiles, ncols,
        tr.enc)


def _check_unit(dev, path, cols, tags):
    """cols: name -> (numpy values, null mask or None). A PLAIN int32
    column `p` is written in front, so the raw pages sit at a non-zero
    offset of the values buffer. tags: name -> expected UD_ENC."""
    from lakesoul_amd.ops import cpp

    names = ["p"] + list(cols)
    raw = ec.read_unit_gpu_route([path], names)
    desc = raw["desc"].numpy()
    assert desc[0, cpp().UD_ENC] == 0
    for u, name in enumerate(names[1:], 1):
        assert desc[u, cpp().UD_ENC] == tags[name] != 0, (name, desc[u])
        assert desc[u, cpp().UD_VAL_OFF] > 0
    outs = _decode(dev, raw, 1, len(names))
    n = len(next(iter(cols.values()))[0])
    np.testing.assert_array_equal(
        outs[0][0].view(torch.int32).cpu().numpy(), np.arange(n, dtype=np.int32))
    for u, name in enumerate(names[1:], 1):
        v, mask = cols[name]
        want = ec.bits(v)
        data, valid = outs[u]
        got = data.cpu().numpy().view(want.dtype)
        assert len(got) == n, name
        if mask is None or not mask.any():
            assert valid is None, name
            np.testing.assert_array_equal(got, want, err_msg=name)
        else:
            np.testing.assert_array_equal(valid.cpu().numpy().astype(bool), ~mask,
                                          err_msg=name)
            np.testing.assert_array_equal(got[~mask], want[~mask], err_msg=name)


def _write(path, cols, encs, version, codec, **kw):
    n = len(next(iter(cols.values()))[0])
    arrays = {"p": pa.array(np.arange(n, dtype=np.int32))}
    arrays.update({k: pa.array(v, mask=m) for k, (v, m) in cols.items()})
    return ec.write(path, arrays, dict(encs, p="PLAIN"), version, codec, **kw)


@pytest.mark.parametrize("version,codec", [("1.0", "none"), ("2.0", "zstd")])
@pytest.mark.parametrize("optional", [False, True], ids=["required", "optional"])
def test_delta_binary_decode_gpu(dev, tmp_path, version, codec, optional):
    """Every boundary row count of the 256/4 (int64) and 128/4 (int32)
    layouts; widths 0, 32, 64, growing widths, wraparound, full range."""
    from lakesoul_amd.ops import cpp

    for np_dtype, counts in ((np.int64, ec.INT64_COUNTS),
                             (np.int32, ec.INT32_COUNTS)):
        for n in counts:
            cols = {k: (v, ec.null_mask(n, "some", n + i) if optional else None)
                    for i, (k, v) in enumerate(
                        ec.int_value_sets(np_dtype, n, seed=n).items())}
            path = _write(tmp_path / f"dbp_{np.dtype(np_dtype).name}_{n}.parquet",
                          cols, {k: "DELTA_BINARY_PACKED" for k in cols},
                          version, codec)
            _check_unit(dev, path, cols,
                        {k: cpp().UD_ENC_DELTA_BINARY for k in cols})


@pytest.mark.parametrize("version,codec", [("1.0", "snappy"), ("2.0", "none")])
@pytest.mark.parametrize("optional", [False, True], ids=["required", "optional"])
def test_byte_stream_split_decode_gpu(dev, tmp_path, version, codec, optional):
    from lakesoul_amd.ops import cpp

    for n in ec.BSS_COUNTS:
        values = {
            "f32": ec.float_specials(np.float32, n, n),
            "f64": ec.float_specials(np.float64, n, n + 1),
            "i32": ec.int_value_sets(np.int32, n, n)["random"],
            "i64": ec.int_value_sets(np.int64, n, n)["random"],
        }
        cols = {k: (v, ec.null_mask(n, "some", n + i) if optional else None)
                for i, (k, v) in enumerate(values.items())}
        path = _write(tmp_path / f"bss_{n}.parquet", cols,
                      {k: "BYTE_STREAM_SPLIT" for k in cols}, version, codec)
        _check_unit(dev, path, cols,
                    {k: cpp().UD_ENC_BYTE_STREAM_SPLIT for k in cols})


@pytest.mark.parametrize("version", ec.VERSIONS)
@pytest.mark.parametrize("null_kind", [None, "page"], ids=["required", "nulls"])
def test_multi_page_multi_chunk_gpu(dev, tmp_path, version, null_kind):
    """Several pages per chunk, three chunks; with nulls: ~30 %, a row
    group whose pages are entirely null, a column that is entirely null.
    The page counts come from the unit's own page table."""
    import pyarrow.parquet as pq

    from lakesoul_amd.ops import cpp

    cols, encs = ec.multi_columns(null_kind)
    path = _write(tmp_path / "multi.parquet", cols, encs, version, "zstd",
                  **ec.MULTI_KW)
    nchunks = pq.ParquetFile(path).metadata.num_row_groups
    assert nchunks > 1
    desc = ec.read_unit_gpu_route([path], ["a", "f"])["desc"].numpy()
    assert (desc[:, cpp().UD_ENC_PAGES] > 2 * nchunks).all(), desc
    tags = {k: cpp().UD_ENC_DELTA_BINARY if e.startswith("DELTA")
            else cpp().UD_ENC_BYTE_STREAM_SPLIT for k, e in encs.items()}
    _check_unit(dev, path, cols, tags)


def test_mixed_files_in_one_unit_gpu(dev, tmp_path):
    """Same column in one unit: a PLAIN file, a DELTA_BINARY_PACKED file,
    a file without it."""
    from lakesoul_amd.ops import cpp

    n = 300
    a = ec.int_value_sets(np.int64, n, 1)["random"]
    b = ec.int_value_sets(np.int64, n, 2)["random"]
    files = [
        ec.write(tmp_path / "plain.parquet", {"x": pa.array(a)}, {"x": "PLAIN"}),
        ec.write(tmp_path / "delta.parquet", {"x": pa.array(b)},
                 {"x": "DELTA_BINARY_PACKED"}),
        ec.write(tmp_path / "none.parquet", {"y": pa.array(a)}, {"y": "PLAIN"}),
    ]
    raw = ec.read_unit_gpu_route(files, ["x"])
    assert raw["desc"][:, cpp().UD_ENC].tolist() == [0, cpp().UD_ENC_DELTA_BINARY, 0]
    outs = _decode(dev, raw, 3, 1)
    np.testing.assert_array_equal(outs[0][0].view(torch.int64).cpu().numpy(), a)
    np.testing.assert_array_equal(outs[1][0].view(torch.int64).cpu().numpy(), b)
    assert outs[2] is None


def test_dictionary_fallback_chunk_gpu(dev, tmp_path):
    """A dictionary chunk with fallback pages next to a dictionary-only row
    group: a plain column through the GPU decoder."""
    path, a, s = ec.write_dict_fallback(tmp_path / "fallback.parquet", "zstd")
    raw = ec.read_unit_gpu_route([path], ["a", "s"])
    outs = _decode(dev, raw, 1, 2)
    np.testing.assert_array_equal(outs[0][0].view(torch.int64).cpu().numpy(), a)
    offs, by, valid = outs[1]
    assert valid is None
    offs, by = offs.cpu().numpy(), by.cpu().numpy().tobytes()
    assert [by[offs[i]:offs[i + 1]].decode() for i in range(len(s))] == s


def test_env_forces_host_route(dev, tmp_path):
    """The production fetch (reader_gpu.fetch_raw) takes the GPU route by
    default; with LAKESOUL_GPU_DELTA=0, in a fresh process, it does not,
    and the decoded values are the same."""
    from lakesoul_amd.io.reader_gpu import fetch_raw
    from lakesoul_amd.ops import cpp

    n = 258
    a = ec.int_value_sets(np.int64, n, 1)["random"]
    f = ec.float_specials(np.float32, n, 2)
    mask = ec.null_mask(n, "some", 3)
    path = ec.write(tmp_path / "env.parquet",
                    {"a": pa.array(a, mask=mask), "f": pa.array(f)},
                    {"a": "DELTA_BINARY_PACKED", "f": "BYTE_STREAM_SPLIT"})
    raw = fetch_raw([path], ["a", "f"])
    assert raw["desc"][:, cpp().UD_ENC].tolist() == [
        cpp().UD_ENC_DELTA_BINARY, cpp().UD_ENC_BYTE_STREAM_SPLIT]
    outs = _decode(dev, raw, 1, 2)

    out = str(tmp_path / "child.npz")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                         "gpu_encodings_child.py")
    env = dict(os.environ, LAKESOUL_GPU_DELTA="0")
    r = subprocess.run([sys.executable, child, out, "a,f", path], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = np.load(out)
    assert res["enc"].tolist() == [0, 0]
    for u, want in enumerate((a, f)):
        got = outs[u][0].cpu().numpy()
        np.testing.assert_array_equal(res[f"data{u}"], got)
        if u == 0:
            np.testing.assert_array_equal(res["valid0"], outs[0][1].cpu().numpy())
            np.testing.assert_array_equal(res["valid0"].astype(bool), ~mask)
            np.testing.assert_array_equal(got.view(np.int64)[~mask], a[~mask])
        else:
            np.testing.assert_array_equal(got.view(np.uint32), ec.bits(f))


def _count_calls(monkeypatch, owner, name):
    calls = []
    real = getattr(owner, name)

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(owner, name, spy)
    return calls


@pytest.mark.parametrize("pks", [["id"], ["id", "id2"]],
                         ids=["fast_path", "generic_path"])
def test_gpu_foreign_encodings_mor(dev, tmp_path, monkeypatch, pks):
    """A foreign file with DELTA_BINARY_PACKED keys and values, a
    BYTE_STREAM_SPLIT and a DELTA_BYTE_ARRAY column merged with an upsert of
    ours: scan(cuda) == scan(cpu) == the expected frame. The single int64
    PK takes the one-call unit path on delta-encoded keys."""
    import lakesoul_amd._hip as hipmod

    t, exp, (fid, fc, cmask) = ec.foreign_table(
        tmp_path, ec.mk_catalog(tmp_path), pks)
    calls = _count_calls(monkeypatch, hipmod, "scan_unit_uselast")
    gpu = t.scan(device="cuda").to_arrow().sort_by("id")
    if pks == ["id"]:
        assert calls, "scan did not take the one-call unit path"
    else:
        assert not calls
    cpu = t.scan(device="cpu").to_arrow().sort_by("id")
    assert gpu.column("c").to_pylist() == cpu.column("c").to_pylist()
    by_id = dict(zip(gpu.column("id").to_pylist(), gpu.column("c").to_pylist()))
    for i, x, isnull in zip(fid.tolist(), fc.tolist(), cmask.tolist()):
        assert by_id[i] == (None if isnull else x), i
    cols = ["id", "id2", "v", "s"]
    g = ec.frame_bits(gpu.to_pandas()[cols])
    assert g == ec.frame_bits(cpu.to_pandas()[cols])
    assert g == ec.frame_bits(exp[cols])


def test_gpu_foreign_encodings_sum_all(dev, tmp_path):
    """SumAll on a DELTA_BINARY_PACKED value column."""
    t, exp, (fid, fc, _) = ec.foreign_table(
        tmp_path, ec.mk_catalog(tmp_path), ["id"], name="foreign_sum",
        properties={"merge_op.c": "SumAll"}, c_nulls=False)
    gpu = t.scan(device="cuda").to_arrow().sort_by("id")
    cpu = t.scan(device="cpu").to_arrow().sort_by("id")
    assert gpu.column("c").to_pylist() == cpu.column("c").to_pylist()
    n = 3000
    want = {i: 1 for i in range(n)}
    for i, x in zip(fid.tolist(), fc.tolist()):
        want[i] = want.get(i, 0) + x
    assert dict(zip(gpu.column("id").to_pylist(),
                    gpu.column("c").to_pylist())) == want
    cols = ["id", "id2", "v", "s"]
    assert ec.frame_bits(gpu.to_pandas()[cols]) == ec.frame_bits(exp[cols])


def test_gpu_foreign_string_pk(dev, tmp_path):
    """A DELTA_BYTE_ARRAY string primary key through the GPU scan."""
    from lakesoul_amd.io.schema import Field, Schema

    t = ec.mk_catalog(tmp_path).create_table(
        "gspk", Schema([Field("k", "string", False), Field("v", "int64")]),
        primary_keys=["k"], hash_bucket_num=1)
    n, m = 1000, 300
    keys = [f"org/unit/key-{i:06d}" for i in range(n)]
    t.upsert({"k": keys, "v": np.zeros(n, dtype=np.int64)}, device="cpu")
    fkeys = keys[:m] + [f"org/unit/new-{i:06d}" for i in range(50)]
    fv = np.arange(1, len(fkeys) + 1, dtype=np.int64)
    foreign = ec.write(
        tmp_path / "part-foreign0000000_0000.parquet",
        {"k": pa.array(fkeys, type=pa.string()), "v": pa.array(fv)},
        {"k": "DELTA_BYTE_ARRAY", "v": "DELTA_BINARY_PACKED"}, "2.0", "snappy",
        data_page_size=1024, write_batch_size=64)
    ec.commit_foreign(t, foreign)
    gpu = t.scan(device="cuda").to_arrow().sort_by("k")
    want = {k: 0 for k in keys}
    want.update(dict(zip(fkeys, fv.tolist())))
    assert gpu.column("k").to_pylist() == sorted(want)
    assert gpu.column("v").to_pylist() == [want[k] for k in sorted(want)]
