"""The GPU string route on the host side (no GPU needed): the layout that
read_unit_raw(gpu_strings=True) produces (UD_STR), decoded with the _cpp
twins of the two kernels; the twins on the hand-built tables of the direct
GPU tests; the two prefix walks on damaged input; the sanitizer program.
Every comparison is byte-exact against the Python lists the files were
written from. Without the feature the tests fail at gpu_strings=True,
UD_STR and the missing bindings."""

import os
import shutil
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

import encoding_cases as ec
import string_cases as sc


def _check_file(path, cols, tags, names=None):
    """cols: name -> (list of str, mask). Tags asserted per string column;
    the GPU-route layout decoded with the twins == the host route == the
    inputs."""
    from lakesoul_amd.ops import cpp

    names = names or ["p"] + list(cols)
    raw = sc.read_unit_strings([path], names)
    host = sc.read_unit_strings([path], names, gpu_strings=False)
    assert host["desc"][:, cpp().UD_STR].tolist() == [0] * len(names)
    for u, name in enumerate(names):
        if name == "p":
            assert int(raw["desc"][u, cpp().UD_STR]) == 0
            continue
        tag = int(raw["desc"][u, cpp().UD_STR])
        want_tag = tags[name]
        assert tag in want_tag if isinstance(want_tag, tuple) else tag == want_tag, \
            (name, tag, want_tag)
        if tag:
            assert int(raw["desc"][u, cpp().UD_VAL_OFF]) > 0
        vals, mask = cols[name]
        want = sc.expected(vals, mask)
        got = sc.unit_string_column_any(raw, u)
        assert got == want, name
        assert ec.unit_string_column(host, u) == want, name


@pytest.mark.parametrize("codec", ec.CODECS)
@pytest.mark.parametrize("version", ec.VERSIONS)
@pytest.mark.parametrize("encoding", sc.STRING_ENCODINGS)
def test_layout_pyarrow_files(tmp_path, encoding, version, codec):
    """string_sets(), required and with ~30 % nulls, in each encoding."""
    tag = sc.expected_tag(encoding)
    for name, vals in ec.string_sets().items():
        n = len(vals)
        cols = {"s": (vals, None), "sn": (vals, ec.null_mask(n, "some", n))}
        path = sc.write_strings(tmp_path / f"{name}.parquet", cols, encoding,
                                version, codec)
        _check_file(path, cols, {"s": tag, "sn": tag})


@pytest.mark.parametrize("encoding", sc.STRING_ENCODINGS)
def test_layout_multi_page_multi_chunk(tmp_path, encoding):
    """Several pages per chunk, three chunks, a whole row group null, an
    all-null column (which holds no value of either kind)."""
    from lakesoul_amd.ops import cpp

    cols = sc.multi_string_columns()
    path = sc.write_strings(tmp_path / "multi.parquet", cols, encoding, "2.0",
                            "zstd", **ec.MULTI_KW)
    assert pq.ParquetFile(path).metadata.num_row_groups == 3
    tag = sc.expected_tag(encoding)
    _check_file(path, cols, {"keys": tag, "low": tag,
                             "allnull": (cpp().UD_STR_PLAIN, cpp().UD_STR_DICT)})


def test_layout_project_file(tmp_path):
    from lakesoul_amd.ops import cpp

    vals = ec.string_sets()["unicode"] * 9  # 2700 rows: three row groups
    mask = ec.null_mask(len(vals), "some", 4)
    path = sc.write_project_file(tmp_path / "ours.parquet", vals, mask)
    assert pq.ParquetFile(path).metadata.num_row_groups == 3
    _check_file(path, {"s": (vals, None), "sn": (vals, mask)},
                {"s": cpp().UD_STR_PLAIN, "sn": cpp().UD_STR_PLAIN})


def test_mixed_and_list_columns_stay_on_the_host(tmp_path):
    """A dictionary row group next to a fallen-back one, and list<string>:
    UD_STR == 0, and the same values as ever."""
    from lakesoul_amd.ops import cpp

    path, a, s = ec.write_dict_fallback(tmp_path / "fallback.parquet", "zstd")
    raw = sc.read_unit_strings([path], ["a", "s"])
    assert raw["desc"][:, cpp().UD_STR].tolist() == [0, 0]
    assert ec.unit_string_column(raw, 1) == [x.encode() for x in s]

    lists = [["a", "bc"], [], None, ["", "def"]] * 10
    lp = str(tmp_path / "list.parquet")
    pq.write_table(pa.table({"l": pa.array(lists, type=pa.list_(pa.string()))}),
                   lp, use_dictionary=False)
    raw = sc.read_unit_strings([lp], ["l"])
    host = sc.read_unit_strings([lp], ["l"], gpu_strings=False)
    assert raw["desc"][:, cpp().UD_STR].tolist() == [0]
    for k in ("values", "soffs", "validity"):
        assert torch.equal(raw[k], host[k]), k


def test_three_file_unit_layout(tmp_path):
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
    assert raw["desc"][:, cpp().UD_PRESENT].tolist() == [1, 1, 0]
    assert sc.unit_string_column_any(raw, 0) == [x.encode() for x in a]
    assert sc.unit_string_column_any(raw, 1) == [x.encode() for x in b]


# ---- the twins on the direct tables ----------------------------------- #

def test_strip_prefixes_twin():
    from lakesoul_amd.ops import cpp

    cases = dict(sc.strip_cases(), stride=sc.stride_case())
    for name, vals in cases.items():
        raw, offs = sc.plain_stream(vals)
        got = cpp().strip_prefixes(torch.from_numpy(raw), torch.from_numpy(offs))
        assert got.numpy().tobytes() == b"".join(vals), name


@pytest.mark.parametrize("kind", sc.VALIDITY_KINDS)
def test_dict_strings_twin(kind):
    from lakesoul_amd.ops import cpp

    for nent in sc.DICT_SIZES:
        _, doff, dby = sc.dictionary(nent)
        idx, v, want = sc.dict_rows(nent, 1000, kind)
        offs, by, status = cpp().dict_strings(
            torch.from_numpy(idx), torch.from_numpy(doff), torch.from_numpy(dby),
            None if v is None else torch.from_numpy(v))
        assert int(status[0]) == 0
        assert sc.rows_of(offs.numpy(), by.numpy(), v) == want, nent


def test_dict_strings_twin_bad_index():
    """An index equal to the dictionary size and INT32_MAX: status set,
    those rows empty, the others right."""
    from lakesoul_amd.ops import cpp

    nent = 300
    entries, doff, dby = sc.dictionary(nent)
    idx, _, want = sc.dict_rows(nent, 500, "none")
    idx[3], idx[400] = nent, np.iinfo(np.int32).max
    want[3] = want[400] = b""
    offs, by, status = cpp().dict_strings(
        torch.from_numpy(idx), torch.from_numpy(doff), torch.from_numpy(dby))
    assert int(status[0]) != 0
    assert sc.rows_of(offs.numpy(), by.numpy()) == want


# ---- damaged input through the walks ----------------------------------- #

def _stream(values):
    return sc.plain_stream(values)[0].tobytes()


def test_walks_accept_valid_streams():
    from lakesoul_amd.ops import cpp

    vals = sc.strip_cases()["phases"]
    raw, offs = sc.plain_stream(vals)
    assert cpp().str_walk_plain(raw.tobytes(), len(vals)).tolist() == offs.tolist()
    o, by = cpp().str_walk_dict(raw.tobytes(), len(vals))
    assert o.tolist() == offs.tolist()
    assert by.numpy().tobytes() == b"".join(vals)
    assert cpp().str_walk_plain(b"", 0).tolist() == [0]


@pytest.mark.parametrize("walk", ["plain", "dict"])
def test_walks_refuse_damaged_streams(walk):
    from lakesoul_amd.ops import cpp

    fn = cpp().str_walk_plain if walk == "plain" else cpp().str_walk_dict
    good = _stream([b"abc", b"", b"defgh"])
    fn(good, 3)
    damaged = {
        "prefix past the end": (good + b"\x01\x00", 4),
        "length past the end": (_stream([b"abc"]) + (9).to_bytes(4, "little") + b"xy", 2),
        "huge length": (_stream([b"abc"]) + b"\xff\xff\xff\xff", 2),
        "one value too few": (good, 4),
        "trailing bytes": (good + b"z", 3),
        "one value too many": (good, 2),
        "negative count": (good, -1),
    }
    for name, (stream, n) in damaged.items():
        with pytest.raises(RuntimeError):
            fn(stream, n)
    # every truncation of a valid stream is refused
    for cut in range(len(good)):
        with pytest.raises(RuntimeError):
            fn(good[:cut], 3)


def _patch_file(src, dst, old, new):
    data = open(src, "rb").read()
    assert data.count(old) == 1, data.count(old)
    open(dst, "wb").write(data.replace(old, new))
    return str(dst)


def test_damaged_dictionary_files_are_refused(tmp_path):
    """A dictionary page shorter than dict_num_values, and an RLE run whose
    value equals the dictionary size: read_unit_raw(gpu_strings=True)
    raises."""
    vals = ["aaaa"] * 100 + ["bbbbbb"] * 100
    good = str(tmp_path / "good.parquet")
    pq.write_table(pa.table({"s": pa.array(vals, type=pa.string())}).cast(
        pa.schema([pa.field("s", pa.string(), nullable=False)])), good,
        use_dictionary=True, compression="none", data_page_version="1.0")
    raw = sc.read_unit_strings([good], ["s"])
    assert sc.unit_string_column_any(raw, 0) == [v.encode() for v in vals]

    # index page: bit width 1, RLE run of 100 x 0, RLE run of 100 x 1
    runs = b"\x01\xc8\x01\x00\xc8\x01\x01"
    bad = _patch_file(good, tmp_path / "run.parquet", runs, runs[:-1] + b"\x02")
    with pytest.raises(RuntimeError, match="dictionary index out of range"):
        sc.read_unit_strings([bad], ["s"])

    # dictionary page: the second entry announces more bytes than are left
    page = b"\x04\x00\x00\x00aaaa\x06\x00\x00\x00bbbbbb"
    bad = _patch_file(good, tmp_path / "dict.parquet", page,
                      page.replace(b"\x06\x00\x00\x00", b"\x07\x00\x00\x00"))
    with pytest.raises(RuntimeError, match="dictionary page"):
        sc.read_unit_strings([bad], ["s"])
    # ... and one whose first entry swallows the second: fewer entries than
    # dict_num_values
    bad = _patch_file(good, tmp_path / "dict2.parquet", page,
                      page.replace(b"\x04\x00\x00\x00", b"\x0e\x00\x00\x00"))
    with pytest.raises(RuntimeError, match="dictionary page"):
        sc.read_unit_strings([bad], ["s"])


def test_str_walk_sanitizer_clean(tmp_path):
    """The two walks and the two twins under AddressSanitizer + UBSan on
    exactly-sized heap buffers (csrc/cpp/tests/str_walk_san.cc)."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "csrc", "cpp", "tests", "str_walk_san.cc")
    exe = str(tmp_path / "str_walk_san")
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
