"""Write path: hash-bucket scatter + PK sort + parquet encode.

MI355X-native analog of the reference writer stack
(``rust/lakesoul-io/src/writer/mod.rs:83-151``): for PK tables the batch
is bucketed by spark-murmur3 (bit-exact, ``utils/hash/``), sorted by PK
(SortAsyncWriter analog, ``sort_writer.rs:35-151``), and each bucket is
written as ``{prefix}/part-{rand16}_{bucket:04}.parquet``
(``writer/mod.rs:119-125``). Range partitions fan out to ``col=val/``
subdirectories (PartitioningAsyncWriter analog,
``partitioning_writer.rs:248-330``).

On GPU, hashing/sort/partition run as HIP kernels on HBM-resident
columns; encode is host-side (zstd(1), dict off — writer/mod.rs:224-245).
"""

from __future__ import annotations

import os
import random
import string as _string
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import constants
from ..ops import cpp
from ..utils import timing
from .batch import Batch, Column
from .fs import default_fs, is_remote
from .schema import Schema

_CODEC_ID = {"zstd": 6, "none": 0, "uncompressed": 0,
             "lz4_raw": 7, "lz4": 7}  # pyarrow's names for LZ4_RAW


@dataclass
class FlushResult:
    path: str
    size: int
    rows: int
    partition_desc: str
    exist_cols: str


def random_str(n: int = 16) -> str:
    return "".join(random.choices(_string.ascii_lowercase + _string.digits, k=n))


def _hash_bucket_ids(batch: Batch, pk: Sequence[str], num_buckets: int) -> torch.Tensor:
    """Spark-murmur3 bucket ids, seed-chained over PK columns."""
    dev = None
    for name in pk:
        c = batch.columns[name]
        t = c.data if not c.is_string else c.bytes_
        if t is not None and t.device.type == "cuda":
            dev = t.device
    if dev is not None:
        from ..ops import hip

        hashes = None
        for i, name in enumerate(pk):
            c = batch.columns[name]
            if c.is_string:
                hashes = hip().hash_string_column(
                    c.offsets.to(dev).to(torch.int32),
                    c.bytes_.to(dev),
                    c.validity.to(dev) if c.validity is not None else torch.empty(0, dtype=torch.uint8, device=dev),
                    hashes if hashes is not None else torch.empty(0, dtype=torch.int64, device=dev),
                    i == 0,
                )
            else:
                hashes = hip().hash_fixed_column(
                    c.data.to(dev),
                    c.validity.to(dev) if c.validity is not None else torch.empty(0, dtype=torch.uint8, device=dev),
                    hashes if hashes is not None else torch.empty(0, dtype=torch.int64, device=dev),
                    i == 0,
                )
        return hip().bucket_ids(hashes, num_buckets)
    # CPU: native host impl
    hashes = None
    first = True
    fixed_cols: List[torch.Tensor] = []
    # mixed fixed/string requires stepwise chaining
    for i, name in enumerate(pk):
        c = batch.columns[name]
        if c.is_string:
            hashes = cpp().hash_string_column_cpu(
                c.offsets, c.bytes_, c.validity, hashes, i == 0
            )
        else:
            t = c.data
            if t.dtype == torch.uint8:
                t = t.to(torch.bool)
            h = cpp().hash_columns_cpu([t], [c.validity])
            if i == 0:
                hashes = h
            else:
                # chain: re-hash col i with seed=hashes — hash_columns_cpu
                # only supports fresh seed, so use the step API
                hashes = cpp().hash_columns_chain_cpu([t], [c.validity], hashes) if hasattr(cpp(), "hash_columns_chain_cpu") else _chain_cpu(t, c.validity, hashes)
        first = False
    return cpp().bucket_ids_from_hashes(hashes, num_buckets)


def _chain_cpu(t: torch.Tensor, validity, prev: torch.Tensor) -> torch.Tensor:
    """Chain a fixed-width column into existing hashes (CPU, numpy)."""
    from ..utils import murmur3_np as m3

    seeds = prev.numpy().astype(np.uint32)
    npv = t.numpy()
    if npv.dtype == np.uint8:  # bool storage
        npv = npv.astype(np.uint32)
    new = m3.hash_column(npv, seeds)
    if validity is not None:
        mask = validity.numpy().astype(bool)
        new = np.where(mask, new, seeds)
    return torch.from_numpy(new.astype(np.int64))


def _sort_indices(batch: Batch, sort_cols: Sequence[str]) -> torch.Tensor:
    """Stable sort by sort_cols (first = primary)."""
    n = batch.num_rows
    first_col = batch.columns[sort_cols[0]]
    dev_t = first_col.data if not first_col.is_string else first_col.bytes_
    if dev_t is not None and dev_t.device.type == "cuda":
        if not any(batch.columns[c].is_string for c in sort_cols):
            idx = torch.arange(n, dtype=torch.int64, device=dev_t.device)
            for name in reversed(sort_cols):
                keys = batch.columns[name].data[idx]
                order = torch.argsort(keys, stable=True)
                idx = idx[order]
            return idx
        # string sort keys: order computed on host (lexicographic byte
        # compare), applied on device
        cpu_batch = batch.to_device("cpu")
        return _sort_indices(cpu_batch, sort_cols).to(dev_t.device)
    # CPU: numpy lexsort
    keys = [np.arange(n)]
    for name in reversed(sort_cols):
        c = batch.columns[name]
        if c.is_string:
            b = c.bytes_.numpy().tobytes()
            o = c.offsets.numpy()
            keys.append(np.array([b[o[i]:o[i + 1]] for i in range(n)], dtype=object))
        else:
            keys.append(c.data.numpy())
    order = np.lexsort(tuple(keys))
    return torch.from_numpy(order)


def _partition_descs(batch: Batch, range_cols: Sequence[str]):
    """Group rows by range-partition values.

    Returns list of (desc, subdir, row_index_tensor). Desc format
    "col=val,col2=val2" (reference helpers/mod.rs:453-501); non-partitioned
    tables use "-5"."""
    n = batch.num_rows
    if not range_cols:
        return [(constants.NON_PARTITION_TABLE_PART_DESC, "", None)]
    import numpy as _np

    # vectorized grouping: encode each range column to small int codes,
    # combine, then one argsort — no python-per-row loop on the fixed-width
    # path (large range-partitioned writes would otherwise crawl). Values
    # go through encode_partition_value so NULL/''/','/'=' survive the
    # "col=val,col2=val2" desc round trip (reference helpers/mod.rs:206-221;
    # ADVICE r1 high finding).
    codes = _np.zeros(n, dtype=_np.int64)
    encoded_cols = []  # per range col: object ndarray of encoded strings
    for name in range_cols:
        c = batch.columns[name]
        valid = None if c.validity is None else c.validity.cpu().numpy().astype(bool)
        if c.is_string:
            b = c.bytes_.cpu().numpy().tobytes()
            o = c.offsets.cpu().numpy()
            enc = _np.array(
                [constants.encode_partition_value(
                    None if (valid is not None and not valid[i])
                    else b[o[i]:o[i + 1]].decode())
                 for i in range(n)], dtype=object)
        else:
            raw = c.data.cpu().numpy()
            enc = raw.astype(str).astype(object)
            if valid is not None and not valid.all():
                enc[~valid] = constants.LAKESOUL_NULL_STRING
        encoded_cols.append(enc)
        uniq, inv = _np.unique(enc, return_inverse=True)
        codes = codes * (len(uniq) + 1) + inv
    uniq_codes, inv_codes = _np.unique(codes, return_inverse=True)
    order = _np.argsort(inv_codes, kind="stable")
    bounds = _np.searchsorted(inv_codes[order], _np.arange(len(uniq_codes) + 1))
    out = []
    for g in range(len(uniq_codes)):
        rows = order[bounds[g]:bounds[g + 1]]
        i0 = int(rows[0])
        parts = [f"{cname}={encoded_cols[k][i0]}"
                 for k, cname in enumerate(range_cols)]
        desc = ",".join(parts)
        subdir = "/".join(parts)
        out.append((desc, subdir, torch.from_numpy(_np.ascontiguousarray(rows))))
    return out


def _write_batch_to_file(path: str, batch: Batch, compression: str, level: int,
                         row_group_size: int) -> int:
    """Write one parquet file; remote destinations stream row-group parts
    while the next row group encodes (multipart_writer.rs:43 overlap);
    a failure aborts the upload so no partial object becomes visible."""
    if is_remote(path):
        from .multipart import StreamingParquetUpload

        up = StreamingParquetUpload(path, batch.schema, compression, level,
                                    row_group_size)
        try:
            n = batch.num_rows
            cpu_batch = batch.to_device("cpu") if any(
                (c.offsets if (c.is_string or c.is_list) else c.data).device.type
                == "cuda" for c in batch.columns.values()) else batch
            for a in range(0, max(n, 1), max(row_group_size, 1)):
                b = min(a + row_group_size, n)
                with timing.phase("w_encode_stream"):
                    up.write_batch(cpu_batch.slice(a, b))
                if b >= n:
                    break
            with timing.phase("w_upload_tail"):
                return up.close()
        except BaseException:
            up.abort()
            raise
    return _write_batch_to_file_local(path, batch, compression, level, row_group_size)


def marshal_leaf(dtype: str, c) -> tuple:
    """Flatten one leaf column for the C++ writer: (data, offsets,
    elem_offsets)."""
    if c.is_list_str:
        return (c.bytes_.cpu(), c.offsets.cpu().to(torch.int64),
                c.elem_offsets.cpu().to(torch.int32))
    if c.is_list:
        t = c.data.cpu()
        ed = c.elem_dtype
        if ed in ("int8", "int16"):
            t = t.to(torch.int32)
        if ed == "bool":
            t = t.to(torch.uint8)
        return (t, c.offsets.cpu().to(torch.int64), None)
    if c.is_string:
        return (c.bytes_.cpu(), c.offsets.cpu(), None)
    t = c.data.cpu()
    if dtype in ("int8", "int16"):
        t = t.to(torch.int32)  # physical INT32
    if dtype == "bool":
        t = t.to(torch.uint8)
    return (t, None, None)


def expand_schema_leaves(schema):
    """Schema-level leaf expansion matching marshal_batch's ordering:
    (names, dtypes, nullable, parents) per physical parquet leaf."""
    from .schema import map_params, struct_members

    names, dtypes, nullable, parents = [], [], [], []
    for f in schema:
        if f.dtype.startswith("struct<"):
            for n, t in struct_members(f.dtype):
                names.append(n)
                dtypes.append(t)
                nullable.append(f.nullable)
                parents.append(f"struct:{f.name}")
        elif f.dtype.startswith("map<"):
            kt, vt = map_params(f.dtype)
            for role, t in (("key", f"list<{kt}>"), ("value", f"list<{vt}>")):
                names.append(role)
                dtypes.append(t)
                nullable.append(f.nullable)
                parents.append(f"map:{f.name}")
        else:
            names.append(f.name)
            dtypes.append(f.dtype)
            nullable.append(f.nullable)
            parents.append("")
    return names, dtypes, nullable, parents


def marshal_batch(batch: Batch):
    """Expand a batch into the C++ writer's per-leaf arrays. Struct
    members become group leaves (parent 'struct:NAME'); map key/value
    become two list leaves under 'map:NAME' (group validity on both)."""
    from .schema import struct_members

    names, dtypes, columns, offsets, validity, nullable = [], [], [], [], [], []
    elem_offs, parents = [], []

    def emit(name, dtype, c, parent, null_ok, vmask):
        d, o, eo = marshal_leaf(dtype, c)
        names.append(name)
        dtypes.append(dtype)
        columns.append(d)
        offsets.append(o)
        elem_offs.append(eo)
        parents.append(parent)
        nullable.append(null_ok)
        validity.append(None if vmask is None else vmask.cpu())

    for f in batch.schema:
        c = batch.columns[f.name]
        if c.is_struct:
            for mname, _ in struct_members(f.dtype):
                ch = c.children[mname]
                emit(mname, ch.dtype, ch, f"struct:{f.name}", f.nullable,
                     c.validity)
            continue
        if c.is_map:
            for role in ("key", "value"):
                emit(role, c.children[role].dtype, c.children[role],
                     f"map:{f.name}", f.nullable, c.validity)
            continue
        emit(f.name, f.dtype, c, "", f.nullable, c.validity)
    return names, dtypes, columns, offsets, validity, nullable, elem_offs, parents


def _write_batch_to_file_local(path: str, batch: Batch, compression: str, level: int,
                               row_group_size: int) -> int:
    (names, dtypes, columns, offsets, validity, nullable, elem_offs,
     parents) = marshal_batch(batch)
    return cpp().write_parquet(
        path, names, dtypes, columns, offsets, validity, nullable,
        row_group_size, _CODEC_ID.get(compression, 6), level, elem_offs,
        parents,
    )


def write_table_data(table, data, device: Optional[str] = None,
                     compact: bool = False) -> List[FlushResult]:
    """Write a batch of data for a table: range-partition fan-out, hash
    bucketing, PK sort, parquet encode. Returns FlushResults for commit."""
    schema = table.schema
    cfg = table.io_config()
    if device is None:
        device = cfg.resolve_device()
    if not isinstance(data, Batch):
        # partial-column writes (schema evolution / partial upsert): the
        # file records only the provided columns; file_exist_cols tells
        # readers what is present (reference: FlushResult exist_cols,
        # async_writer/mod.rs:49)
        provided = None
        if isinstance(data, dict):
            provided = set(data.keys())
        elif type(data).__module__.startswith("pyarrow"):
            provided = set(data.schema.names)
        elif type(data).__module__.startswith("pandas"):
            provided = set(data.columns)
        if provided is not None and provided != set(schema.names()):
            missing_pk = [p for p in table.primary_keys if p not in provided]
            missing_range = [r for r in table.range_keys if r not in provided]
            if missing_pk or missing_range:
                raise ValueError(
                    f"partial write must include pk+range columns, missing {missing_pk + missing_range}"
                )
            schema = schema.select([n for n in schema.names() if n in provided])
        with timing.phase("w_from_any"):
            batch = Batch.from_any(data, schema)
    else:
        batch = data
        schema = batch.schema
    if device is not None and str(device).startswith("cuda"):
        with timing.phase("w_h2d", sync_gpu=True):
            batch = batch.to_device(device)

    pk = table.primary_keys
    range_cols = table.range_keys
    num_buckets = table.hash_bucket_num
    data_schema = Schema([f for f in schema if f.name not in range_cols])

    results: List[FlushResult] = []
    for desc, subdir, rows in _partition_descs(batch, range_cols):
        part_batch = batch if rows is None else batch.take(rows)
        # drop range-partition columns from the file (reference stores them
        # in the directory structure only: writer/mod.rs uniform_schema)
        file_batch = Batch(
            data_schema, {f.name: part_batch.columns[f.name] for f in data_schema}
        )
        out_dir = os.path.join(table.table_path, subdir) if subdir else table.table_path
        if compact:
            out_dir = os.path.join(out_dir, constants.COMPACT_DIR)
        if is_remote(out_dir):
            default_fs().makedirs(out_dir)
        else:
            os.makedirs(out_dir, exist_ok=True)

        if pk:
            # one global stable sort by (bucket, pk): buckets become
            # contiguous PK-sorted slices — a single gather for the whole
            # batch instead of one per bucket
            with timing.phase("w_hash_sort", sync_gpu=True):
                buckets = _hash_bucket_ids(file_batch, pk, num_buckets)
                order = _sort_indices(file_batch, pk)
                border = torch.argsort(buckets.to(torch.int64)[order], stable=True)
                perm = order[border]
                sorted_batch = file_batch.take(perm)
            bucket_sorted = buckets[perm].to(torch.int64)
            counts = torch.bincount(bucket_sorted, minlength=num_buckets)
            bounds = torch.zeros(num_buckets + 1, dtype=torch.int64)
            torch.cumsum(counts.cpu(), 0, out=bounds[1:].view(-1))
            bounds = bounds.tolist()

            jobs = []
            for b in range(num_buckets):
                a, e = bounds[b], bounds[b + 1]
                if a == e:
                    continue
                bucket_batch = sorted_batch.slice(a, e)
                fname = f"part-{random_str(16)}_{b:04d}.parquet"
                fpath = os.path.join(out_dir, fname)
                jobs.append((fpath, bucket_batch))

            from concurrent.futures import ThreadPoolExecutor

            def _encode(job):
                fpath, bb = job
                size = _write_batch_to_file(
                    fpath, bb, cfg.compression, cfg.compression_level,
                    cfg.max_row_group_size,
                )
                return FlushResult(fpath, size, bb.num_rows, desc,
                                   ",".join(data_schema.names()))

            with timing.phase("w_encode"):
                with ThreadPoolExecutor(max_workers=min(16, max(1, len(jobs)))) as ex:
                    results.extend(ex.map(_encode, jobs))
        else:
            fname = f"part-{random_str(16)}_{0:04d}.parquet"
            fpath = os.path.join(out_dir, fname)
            size = _write_batch_to_file(
                fpath, file_batch, cfg.compression, cfg.compression_level,
                cfg.max_row_group_size,
            )
            results.append(
                FlushResult(fpath, size, file_batch.num_rows, desc,
                            ",".join(data_schema.names()))
            )
    return results
