"""Shared inputs of test_string_route.py (CPU) and test_gpu_strings.py (GPU):
hand-built tables for the two string kernels and their host twins, the
pyarrow / project files of the GPU string route, and a host decoder of a
unit's raw buffers built on the _cpp twins."""

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

import encoding_cases as ec

TILE = 4096  # output bytes per workgroup trip of strings.hip


# ---- strip_prefixes --------------------------------------------------- #

def _values(lengths, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(1, 256, int(n), dtype=np.uint8).tobytes() for n in lengths]


def strip_cases():
    """name -> list of bytes values. Lengths 0..17 in an order that starts
    and ends values at every phase of an 8-byte word; values around the
    tile size; one value over many tiles; a run of empties longer than any
    LDS stage of offsets; no bytes at all; no values; an odd total."""
    phases = [(i * 7 + i // 18) % 18 for i in range(18 * 18)]
    cases = {
        "phases": _values(phases, 1),
        "tile": _values([TILE - 1, TILE, TILE + 1, 1, TILE, TILE - 1, 0, 3], 2),
        "long": _values([3, 70000, 5], 3),
        "empties": _values([7] + [0] * 5000 + [9], 4),
        "all_empty": _values([0] * 100, 5),
        "none": [],
        "odd_total": _values([5, 6], 6),
    }
    assert sum(map(len, cases["odd_total"])) % 8 != 0
    return cases


def stride_case():
    """About 12 MB in 300k values: more tiles than the 2048-workgroup grid."""
    n = 300_000
    lengths = 20 + (np.arange(n) * 7) % 41
    blob = np.random.default_rng(7).integers(0, 256, int(lengths.sum()),
                                             dtype=np.uint8).tobytes()
    ends = np.cumsum(lengths)
    return [blob[e - l:e] for e, l in zip(ends.tolist(), lengths.tolist())]


def plain_stream(values):
    """values -> (PLAIN stream uint8 array, dense offsets int64 array)."""
    raw = b"".join(len(v).to_bytes(4, "little") + v for v in values)
    offs = np.zeros(len(values) + 1, dtype=np.int64)
    if values:
        offs[1:] = np.cumsum([len(v) for v in values])
    return np.frombuffer(raw, dtype=np.uint8).copy(), offs


# ---- dict_strings ----------------------------------------------------- #

ENTRY_LENGTHS = [0, 1, 7, 8, 9]
DICT_SIZES = [1, 2, 3, 300, 5000]
VALIDITY_KINDS = ["none", "ends", "all", "some"]


def dictionary(nent, seed=0):
    """nent entries of lengths 0, 1, 7, 8, 9 in turn; dictionaries of 300
    entries and more carry one entry of 5000 bytes. Returns (entries,
    offsets int64, stripped bytes uint8)."""
    lengths = [ENTRY_LENGTHS[(i + seed) % len(ENTRY_LENGTHS)] for i in range(nent)]
    if nent >= 300:
        lengths[17] = 5000
    entries = _values(lengths, 100 + nent + seed)
    offs = np.zeros(nent + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lengths)
    by = np.frombuffer(b"".join(entries), dtype=np.uint8).copy()
    return entries, offs, by


def validity_mask(nrows, kind, seed=0):
    """uint8 validity (1 = valid) or None."""
    if kind == "none":
        return None
    v = np.ones(nrows, dtype=np.uint8)
    if kind == "ends":
        v[0] = v[-1] = 0
    elif kind == "all":
        v[:] = 0
    else:
        v[np.random.default_rng(seed + 5).random(nrows) < 0.3] = 0
    return v


def dict_rows(nent, nrows, kind, seed=0):
    """(dense idx int32, validity or None, expected list of bytes/None)."""
    entries, _, _ = dictionary(nent)
    v = validity_mask(nrows, kind, seed)
    nvalid = nrows if v is None else int(v.sum())
    idx = np.random.default_rng(seed + nent).integers(0, nent, nvalid).astype(np.int32)
    if nent >= 300 and nvalid:
        idx[nvalid // 2] = 17  # the 5000-byte entry
    it = iter(idx.tolist())
    want = [entries[next(it)] if v is None or v[r] else None for r in range(nrows)]
    return idx, v, want


def rows_of(offsets, by, validity=None):
    """(offsets, bytes[, validity]) arrays -> list of bytes/None."""
    offsets = np.asarray(offsets)
    b = np.asarray(by).tobytes()
    return [None if validity is not None and not validity[i]
            else b[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]


# ---- a unit's raw buffers, decoded on the host ------------------------- #

def expand_runs(raw, u):
    """Dense dictionary indices of unit column u from the runs table (what
    the rle_expand kernel computes)."""
    from lakesoul_amd.ops import cpp

    c = cpp()
    d = raw["desc"][u]
    runs = raw["runs"].numpy().reshape(-1, 6)
    runs = runs[int(d[c.UD_RUN_OFF]):int(d[c.UD_RUN_OFF]) + int(d[c.UD_RUN_CNT])]
    bits = np.unpackbits(raw["values"].numpy(), bitorder="little")
    idx = np.zeros(int(d[c.UD_DENSE_N]), dtype=np.int32)
    for out_off, n, lit, val, bw, bias in runs.tolist():
        if not lit:
            idx[out_off:out_off + n] = val
        elif bw == 0:
            idx[out_off:out_off + n] = bias
        else:
            b = bits[val:val + n * bw].reshape(n, bw).astype(np.int64)
            idx[out_off:out_off + n] = (b << np.arange(bw)).sum(axis=1) + bias
    return idx


def unit_string_column_any(raw, u):
    """Unit string column u as a list of bytes/None, whatever its UD_STR:
    the GPU-route layouts go through the _cpp twins of the kernels."""
    import torch

    from lakesoul_amd.ops import cpp

    c = cpp()
    d = raw["desc"][u]
    kind = int(d[c.UD_STR])
    if kind == 0:
        return ec.unit_string_column(raw, u)
    assert int(d[c.UD_SBYTES_OFF]) == -1
    nv, dn = int(d[c.UD_NUM_VALUES]), int(d[c.UD_DENSE_N])
    so = int(d[c.UD_SOFF_OFF])
    valid = ec.unit_valid(raw, u)
    assert int(valid.sum()) == dn
    if kind == c.UD_STR_PLAIN:
        vo, vl = int(d[c.UD_VAL_OFF]), int(d[c.UD_VAL_LEN])
        doff = raw["soffs"][so:so + dn + 1].contiguous()
        assert int(doff[0]) == 0 and int(doff[dn]) == int(d[c.UD_SBYTES_LEN])
        assert int(d[c.UD_SBYTES_LEN]) + 4 * dn == vl
        by = c.strip_prefixes(raw["values"][vo:vo + vl].contiguous(), doff)
        dense = rows_of(doff.numpy(), by.numpy())
        it = iter(dense)
        return [next(it) if valid[r] else None for r in range(nv)]
    assert kind == c.UD_STR_DICT and int(d[c.UD_IS_DICT]) == 1
    nent = int(d[c.UD_SBYTES_LEN])
    do, dl = int(d[c.UD_DICT_OFF]), int(d[c.UD_DICT_LEN])
    idx = torch.from_numpy(expand_runs(raw, u))
    vt = None if valid.all() else torch.from_numpy(valid.astype(np.uint8))
    offs, by, status = c.dict_strings(
        idx, raw["soffs"][so:so + nent + 1].contiguous(),
        raw["dicts"][do:do + dl].contiguous(), vt)
    assert int(status[0]) == 0
    assert len(offs) == nv + 1
    return rows_of(offs.numpy(), by.numpy(), valid)


def read_unit_strings(paths, names, gpu_strings=True):
    from lakesoul_amd.ops import cpp

    return cpp().read_unit_raw([str(p) for p in paths], names, 0, False,
                               gpu_delta=True, gpu_strings=gpu_strings)


# ---- files ------------------------------------------------------------ #

STRING_ENCODINGS = ["PLAIN", "RLE_DICTIONARY", "DELTA_LENGTH_BYTE_ARRAY",
                    "DELTA_BYTE_ARRAY"]


def write_strings(path, columns, encoding, version="1.0", codec="none", **kw):
    """columns: name -> (list of str, null mask or None). An int32 column
    `p` goes in front, so the string payloads sit at a non-zero offset of
    the values buffer. Every string column in `encoding`."""
    n = len(next(iter(columns.values()))[0])
    arrays = {"p": pa.array(np.arange(n, dtype=np.int32))}
    for k, (vals, mask) in columns.items():
        arrays[k] = pa.array(vals, type=pa.string(),
                             mask=None if mask is None else np.asarray(mask))
    path = str(path)
    if encoding == "RLE_DICTIONARY":
        pq.write_table(pa.table(arrays), path, use_dictionary=list(columns),
                       data_page_version=version, compression=codec, **kw)
        md = pq.ParquetFile(path).metadata
        for rg in range(md.num_row_groups):
            for i in range(1, len(arrays)):
                col = md.row_group(rg).column(i)
                assert col.has_dictionary_page, (rg, i)
        return path
    encs = {k: encoding for k in columns}
    encs["p"] = "PLAIN"
    return ec.write(path, arrays, encs, version, codec, **kw)


def expected(vals, mask):
    return [None if mask is not None and mask[i] else vals[i].encode()
            for i in range(len(vals))]


def expected_tag(encoding):
    from lakesoul_amd.ops import cpp

    return (cpp().UD_STR_DICT if encoding == "RLE_DICTIONARY"
            else cpp().UD_STR_PLAIN)


def multi_string_columns():
    """The multi-page, three-chunk case (ec.MULTI_KW): name -> (values,
    mask). `keys`: distinct ~50-byte values, ~30 % nulls and row group 1
    entirely null; `low`: 7 distinct values, no nulls; `allnull`."""
    n = ec.MULTI_N
    keys = [f"tenant-0001/region-eu-west/bucket-{i // 7:05d}/key-{i:07d}"
            for i in range(n)]
    low = ["AIR", "R", "TRUCK", "", "REG AIR", "MAIL", "SHIP-LONGER"]
    return {
        "keys": (keys, ec.null_mask(n, "page", 31)),
        "low": ([low[(i * i) % 7] for i in range(n)], None),
        "allnull": ([""] * n, ec.null_mask(n, "all")),
    }


def write_project_file(path, vals, mask, row_group_size=1000):
    """The project's own writer (PLAIN, zstd): int32 `p`, required string
    `s`, nullable string `sn` (vals under mask)."""
    import torch

    from lakesoul_amd.ops import cpp

    n = len(vals)

    def col(values):
        by = b"".join(values)
        offs = np.zeros(n + 1, dtype=np.int32)
        offs[1:] = np.cumsum([len(v) for v in values])
        return (torch.from_numpy(np.frombuffer(by, dtype=np.uint8).copy()),
                torch.from_numpy(offs))

    enc = [v.encode() for v in vals]
    s_b, s_o = col(enc)
    sn_b, sn_o = col([b"" if mask[i] else enc[i] for i in range(n)])
    valid = torch.from_numpy((~np.asarray(mask)).astype(np.uint8))
    cpp().write_parquet(
        str(path), ["p", "s", "sn"], ["int32", "string", "string"],
        [torch.arange(n, dtype=torch.int32), s_b, sn_b], [None, s_o, sn_o],
        [None, None, valid], [False, False, True], row_group_size, 6, 1)
    return str(path)
