"""A plain model of the merge-on-read merge, a case generator and the
comparison rules shared by test_merge_model.py (merge_cpu vs the model)
and test_gpu_merge_ops.py (GPU merge vs merge_cpu).

Files are dicts ``name -> python list`` (ints, floats, bytes; ``None`` is
a null), rows sorted by primary key and free to repeat a key.
``model_merge`` itself uses no numpy: a dict of groups and python loops.
"""

import itertools
import math
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np

SUM_OPS = ("SumAll", "SumLast")
JOIN_OPS = ("JoinedAllByComma", "JoinedAllBySemicolon",
            "JoinedLastByComma", "JoinedLastBySemicolon")
LAST_OPS = ("SumLast", "JoinedLastByComma", "JoinedLastBySemicolon")

_INT_BITS = {"int8": 8, "int16": 16, "int32": 32, "int64": 64}
_FLOAT_EPS = {"float32": 2.0 ** -23, "float64": 2.0 ** -52}

# every length class around the 8-byte chunk of the GPU string sort, bytes
# on both sides of 0x80, embedded and trailing NULs
STRING_KEY_ALPHABET = [
    b"", b"a", b"a\x00", b"a\x00\x00", b"\x00", b"\x7f", b"\x80", b"\xff",
    "é".encode(), "日本語".encode(),
    b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefgh\x00", b"abcdefgh\x80",
    b"abcdefghABCDEFGH", b"abcdefghABCDEFGHI", b"abcdefghABCDEFG\xff",
    b"\xff" * 17,
]

CDC_VALUES = [b"delete", b"Delete", b"delet", b"deletee", b"", None,
              b"insert", b"update"]

PK_KINDS = ["int64", "int32", "int16", "int8", "int32+int32", "int8+int16",
            "int64+int64", "string", "int64+string"]
# kinds that pack into one u64 and take the merge-path kernel
PACKED_PK_KINDS = ["int64", "int32", "int16", "int8", "int32+int32",
                   "int8+int16"]


def int_bits(dtype: str) -> Optional[int]:
    if dtype.startswith("decimal"):
        return 64
    return _INT_BITS.get(dtype)


def wrap(x: int, bits: int) -> int:
    """Two's-complement wraparound of a python int to ``bits`` bits."""
    x &= (1 << bits) - 1
    return x - (1 << bits) if x >> (bits - 1) else x


# ---------------------------------------------------------------------- #
# the model


def _groups(files, pk):
    """PK tuple -> [(file index, row index)], files oldest -> newest and
    rows in file order."""
    groups = {}
    for fi, f in enumerate(files):
        for ri in range(len(f[pk[0]])):
            groups.setdefault(tuple(f[p][ri] for p in pk), []).append((fi, ri))
    return groups


def participants(files, rows, name, op, present):
    """Values of column ``name`` that take part in ``op`` for one group."""
    vals = []
    for j, (fi, ri) in enumerate(rows):
        if present is not None and name not in present[fi]:
            continue
        if op in LAST_OPS and j + 1 < len(rows) and rows[j + 1][0] == fi:
            continue  # not the last row of its file within the group
        vals.append(files[fi][name][ri])
    return vals


def _reduce(op, vals):
    if op == "UseLast":
        return vals[-1] if vals else None
    if op == "UseLastNotNull":
        for v in reversed(vals):
            if v is not None:
                return v
        return None
    if any(v is None for v in vals):
        return None
    if op in SUM_OPS:
        return list(vals)  # the addends; compare_to_model sums them
    if op in JOIN_OPS:
        return (b"," if op.endswith("Comma") else b";").join(vals)
    raise ValueError(op)


def model_merge(files, pk, ops=None, present=None, cdc=None):
    """name -> list of merged values, rows sorted by PK tuple (bytes as
    unsigned bytes). A sum column holds the list of addends per row."""
    ops = ops or {}
    names = list(files[0].keys())
    groups = _groups(files, pk)
    out = {name: [] for name in names}
    for key in sorted(groups):
        rows = groups[key]
        merged = {}
        for name in names:
            op = "UseLast" if name in pk else ops.get(name, "UseLast")
            merged[name] = _reduce(
                op, participants(files, rows, name, op, present))
        if cdc is not None and merged[cdc] == b"delete":
            continue
        for name in names:
            out[name].append(merged[name])
    return out


# ---------------------------------------------------------------------- #
# cases


@dataclass
class Case:
    fields: list                   # [(name, dtype)], PK columns first
    pk: List[str]
    files: List[Dict[str, list]]
    present: Optional[List[set]]
    cdc: Optional[str]
    null_p: float

    def names(self):
        return [n for n, _ in self.fields]

    def np_files(self):
        """The files as merge_cpu NpColumn dicts."""
        from lakesoul_amd.io.merge_cpu import NpColumn

        out = []
        for fi, f in enumerate(self.files):
            cols = {}
            for name, dtype in self.fields:
                absent = (self.present is not None
                          and name not in self.present[fi])
                cols[name] = _np_column(NpColumn, dtype, f[name], absent)
            out.append(cols)
        return out

    def device_batches(self, device):
        """The files as Batch/Column objects on ``device``: int64 string
        offsets, uint8 bytes and validity, torch_dtype_for data."""
        import torch

        from lakesoul_amd.io.batch import Batch, Column, torch_dtype_for
        from lakesoul_amd.io.schema import Field, Schema

        schema = Schema([Field(n, d, n not in self.pk) for n, d in self.fields])

        def dev(a):
            return None if a is None else torch.from_numpy(a).to(device)

        batches = []
        for cols in self.np_files():
            dcols = {}
            for name, dtype in self.fields:
                c = cols[name]
                col = Column(dtype, dev(c.data), dev(c.offsets), dev(c.bytes_),
                             dev(c.validity))
                if col.data is not None:
                    assert col.data.dtype == torch_dtype_for(dtype)
                dcols[name] = col
            batches.append(Batch(schema, dcols))
        return batches


def _np_column(NpColumn, dtype, values, absent):
    from lakesoul_amd.io.batch import np_dtype_for

    n = len(values)
    validity = None
    if any(v is None for v in values):
        validity = np.array([v is not None for v in values], dtype=np.uint8)
    if dtype in ("string", "binary"):
        enc = [b"" if v is None else v for v in values]
        offs = np.zeros(n + 1, dtype=np.int64)
        offs[1:] = np.cumsum([len(e) for e in enc])
        bys = np.frombuffer(b"".join(enc), dtype=np.uint8).copy()
        return NpColumn(dtype, None, offs, bys, validity)
    # a column its file lacks is zero-filled as the reader does; a null
    # in a column the file has sits over a non-zero value, which a merge
    # that ignored validity would pick up
    fill = 0 if absent else 1
    data = np.array([fill if v is None else v for v in values],
                    dtype=np_dtype_for(dtype))
    return NpColumn(dtype, data, None, None, validity)


def _int_domain(rng, dtype, n):
    bits = _INT_BITS[dtype]
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    vals = [lo, lo + 1, -1, 0, 1, hi - 1, hi]
    if bits == 64:
        vals.append(1 << 31)
    n = min(n, 200)
    while len(vals) < n:
        v = int(rng.integers(lo, hi, endpoint=True))
        if v not in vals:
            vals.append(v)
    return vals


def _half_domain(rng, dtype, n):
    """One half of a composite key: the sign boundary and both ends."""
    if dtype == "string":
        return list(STRING_KEY_ALPHABET)
    bits = _INT_BITS[dtype]
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    vals = [lo, -1, 0, hi]
    n = min(n, 200)
    while len(vals) < n:
        v = int(rng.integers(lo, hi, endpoint=True))
        if v not in vals:
            vals.append(v)
    return vals


def pk_domain(rng, pk_kind, ndomain):
    """([(name, dtype)], sorted list of PK tuples) for a PK kind."""
    parts = pk_kind.split("+")
    if len(parts) == 1:
        if parts[0] == "string":
            vals = list(STRING_KEY_ALPHABET)
            while len(vals) < ndomain:
                v = rng.integers(0, 256, int(rng.integers(0, 20)),
                                 dtype=np.uint8).tobytes()
                if v not in vals:
                    vals.append(v)
        else:
            vals = _int_domain(rng, parts[0], ndomain)
        return [("k0", parts[0])], sorted((v,) for v in vals)
    per_half = max(5, math.isqrt(ndomain) + 1)
    halves = [_half_domain(rng, p, per_half) for p in parts]
    keys = list(itertools.product(*halves))
    if len(keys) > 2 * ndomain:
        pick = rng.choice(len(keys), ndomain, replace=False)
        keys = [keys[i] for i in pick]
    return [(f"k{i}", p) for i, p in enumerate(parts)], sorted(keys)


def _value_pool(rng, vdtype):
    bits = _INT_BITS.get(vdtype)
    if bits:
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        # both ends several times over, so that sums wrap
        return ([lo, hi] * 3 + [-1, 0, 1, lo + 1, hi - 1]
                + [int(x) for x in rng.integers(lo, hi, 12, endpoint=True)])
    if vdtype.startswith("decimal"):
        return [-10 ** 12 + 1, 10 ** 12 - 1, -1, 0, 1] + [
            int(x) for x in rng.integers(-10 ** 11, 10 ** 11, 12)]
    if vdtype in _FLOAT_EPS:
        # float32-representable normals scaled by 10^k, k in [-3, 3]
        return [float(np.float32(rng.standard_normal() * 10.0 ** k))
                for k in range(-3, 4) for _ in range(4)]
    if vdtype == "bool":
        return [0, 1]
    if vdtype == "string":
        return [b"", b",", b";", b"a,b", b"x;y", b"\x00", b"\xff\x80",
                "日本語".encode(), b"v", b"value", b"0123456789abcdef" * 5] + [
            rng.integers(0, 256, int(rng.integers(1, 12)),
                         dtype=np.uint8).tobytes() for _ in range(6)]
    raise ValueError(vdtype)


def gen_case(rng, pk_kind, vdtype, sizes, null_p, partial, cdc=False,
             ndomain=24) -> Case:
    """One merge input: len(sizes) files over a small PK domain (groups
    span files, keys repeat within a file), one value column ``v`` of
    ``vdtype`` and optionally a CDC column ``rk``.

    null_p: chance of a null per value; a quarter of the keys never get
      one, so that null-free groups exist next to poisoned ones
      (null_p = 1 makes the whole column null).
    partial: None, "odd" (odd-numbered files lack ``v``) or "group" (as
      "odd", and two keys occur in odd-numbered files only, so every file
      of their groups lacks ``v``).
    """
    pk_fields, domain = pk_domain(rng, pk_kind, ndomain)
    pk = [n for n, _ in pk_fields]
    fields = pk_fields + [("v", vdtype)] + ([("rk", "string")] if cdc else [])
    perm = [int(i) for i in rng.permutation(len(domain))]
    lonely = set(perm[:2]) if partial == "group" else set()
    clean = set(perm[2:2 + max(1, len(domain) // 4)])
    pool = _value_pool(rng, vdtype)
    files, present = [], []
    for fi, n in enumerate(sizes):
        lacks_v = partial is not None and fi % 2 == 1
        allowed = [i for i in range(len(domain))
                   if lacks_v or i not in lonely]
        idx = [allowed[int(j)] for j in rng.integers(0, len(allowed), n)]
        if lacks_v and lonely and n:
            idx[0] = min(lonely)
        idx.sort()
        f = {name: [domain[i][c] for i in idx] for c, name in enumerate(pk)}
        if lacks_v:
            f["v"] = [None] * n
        else:
            f["v"] = [
                None if null_p >= 1 or (i not in clean and rng.random() < null_p)
                else pool[int(rng.integers(0, len(pool)))] for i in idx]
        if cdc:
            f["rk"] = [CDC_VALUES[int(rng.integers(0, len(CDC_VALUES)))]
                       for _ in idx]
        files.append(f)
        present.append(set(n_ for n_, _ in fields) - ({"v"} if lacks_v else set()))
    return Case(fields, pk, files, present if partial is not None else None,
                "rk" if cdc else None, null_p)


def assert_input_conditions(case: Case, op: str, partial=None):
    """What makes a case worth running, asserted on its inputs: groups
    that span files, keys repeated within a file, poisoned and clean
    groups side by side. Cases of fewer than 2 files or 30 rows are
    degenerate on purpose and exempt."""
    files, pk = case.files, case.pk
    total = sum(len(f[pk[0]]) for f in files)
    if len(files) < 2 or total < 30:
        return
    groups = _groups(files, pk)
    assert any(len({fi for fi, _ in rows}) >= 2 for rows in groups.values())
    assert any(len(rows) != len({fi for fi, _ in rows})
               for rows in groups.values())
    parts = [participants(files, rows, "v", op, case.present)
             for rows in groups.values()]
    if 0 < case.null_p < 1:
        assert any(None in p for p in parts)
        assert any(p and None not in p for p in parts)
    if case.null_p >= 1:
        assert all(v is None for p in parts for v in p)
    lacking = case.present is not None and any(
        "v" not in p and len(f["v"]) for p, f in zip(case.present, files))
    if lacking and op not in LAST_OPS:
        assert any(len(p) < len(rows)
                   for p, rows in zip(parts, groups.values()))
    if partial == "group":
        assert any(not p for p in parts)


# ---------------------------------------------------------------------- #
# comparison


def columns_to_lists(cols) -> Dict[str, list]:
    """NpColumn dict -> python lists, None under a null (validity None
    means all valid; bytes or data under a null are dropped here and so
    never compared)."""
    out = {}
    for name, c in cols.items():
        if c.is_string:
            out[name] = c.string_list()
        else:
            vals = c.data.tolist()
            if c.validity is not None:
                vals = [v if ok else None
                        for v, ok in zip(vals, c.validity.tolist())]
            out[name] = vals
    return out


def batch_to_lists(batch) -> Dict[str, list]:
    """A (device) Batch -> python lists, via NpColumn."""
    from lakesoul_amd.io.merge_cpu import NpColumn

    def host(t):
        return None if t is None else t.cpu().numpy()

    return columns_to_lists({
        name: NpColumn(c.dtype, host(c.data),
                       None if c.offsets is None else host(c.offsets).astype(np.int64),
                       host(c.bytes_), host(c.validity))
        for name, c in batch.columns.items()})


def _is_float_sum(dtype, op):
    return op in SUM_OPS and dtype in _FLOAT_EPS


def compare_to_model(got, model, fields, ops, pk):
    """Every value of every column against the model. Integer sums equal
    the python sum wrapped to the dtype's width. A float sum of m addends
    of type T obeys |got - fsum(v)| <= m * eps(T) * fsum(|v|): the
    recursive-summation bound (m-1) * u * sum|v| with u = eps/2, doubled;
    it holds for any order of summation."""
    for name, dtype in fields:
        op = "UseLast" if name in pk else ops.get(name, "UseLast")
        g, m = got[name], model[name]
        assert len(g) == len(m), (name, len(g), len(m))
        for i, (a, b) in enumerate(zip(g, m)):
            if b is None:
                assert a is None, (name, i, a)
                continue
            assert a is not None, (name, i, b)
            if op not in SUM_OPS:
                assert a == b, (name, i, a, b)
            elif dtype in _FLOAT_EPS:
                ref = math.fsum(b)
                bound = len(b) * _FLOAT_EPS[dtype] * math.fsum(abs(x) for x in b)
                assert abs(a - ref) <= bound, (name, i, a, ref, bound, len(b))
            else:
                assert a == wrap(sum(b), int_bits(dtype)), (name, i, a, b)


def compare_exact(got, want, fields, ops, pk):
    """Two merge results value by value; float sums are left to
    compare_to_model, since their summation orders differ."""
    for name, dtype in fields:
        op = "UseLast" if name in pk else ops.get(name, "UseLast")
        if _is_float_sum(dtype, op):
            continue
        assert got[name] == want[name], name
