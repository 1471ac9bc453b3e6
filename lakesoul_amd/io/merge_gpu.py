"""GPU merge-on-read engine (HIP kernels, HBM-resident columns).

Mirrors merge_cpu.py semantics exactly (same contract as the reference's
SortedStreamMerger + merge operators); GPU tests compare the two.

Fast path: integer PKs that pack into a u64 order-preserving key use the
hand-written merge-path kernel (csrc/hip/kernels.hip merge_round_kernel,
driven by _hip.merge_sorted_keys) to exploit per-file sortedness — K
files merge in ceil(log2 K) passes.
Generic path: iterated stable argsort (lexsort) on the concatenated keys.
Dedup (UseLast), segmented sums, last-non-null and CDC filtering run as
HIP kernels; payload columns are materialized with one fused multi-column
gather.
"""

from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from ..ops import hip
from .batch import Batch, Column
from .schema import Schema


def _pack_keys_one_file(cols: List[Column]) -> Optional[torch.Tensor]:
    """Order-preserving u64 key per row, or None if not packable."""
    if len(cols) == 1:
        c = cols[0]
        if c.is_string:
            return None
        if c.data.dtype in (torch.int64, torch.int32, torch.int16, torch.int8):
            return hip().pack_key_i64(c.data.to(torch.int64))
    elif len(cols) == 2:
        a, b = cols
        if a.is_string or b.is_string:
            return None
        if a.data.dtype in (torch.int32, torch.int16, torch.int8) and b.data.dtype in (
            torch.int32,
            torch.int16,
            torch.int8,
        ):
            return hip().pack_key_2xi32(a.data.to(torch.int32), b.data.to(torch.int32))
    return None


def _string_sort_tensors(cols: List[Column], device) -> List[torch.Tensor]:
    """Most-significant-first sort keys for a string PK column: 8-byte
    big-endian chunk keys (GPU kernel) then length as the final
    tiebreak. Equality across all returned tensors == string equality,
    and stable LSD passes over them give exact lexicographic order
    (ROADMAP round-2 item pulled into round 1)."""
    # per-row lengths -> absolute offsets of the concatenation
    lens = torch.cat([
        (c.offsets[1:] - c.offsets[:-1]).to(torch.int64).to(device) for c in cols
    ])
    offsets = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=device)
    torch.cumsum(lens, 0, out=offsets[1:])
    bys = torch.cat([c.bytes_.to(device) for c in cols])
    maxlen = int(lens.max().item()) if lens.numel() else 0
    nchunks = max(1, (maxlen + 7) // 8)
    if str(device).startswith("cuda"):
        out = [hip().str_chunk_keys(offsets, bys, ci) for ci in range(nchunks)]
    else:
        # CPU reference of the kernel (tests without a GPU)
        import numpy as np

        n = lens.numel()
        offs_np = offsets.cpu().numpy()
        lens_np = lens.cpu().numpy()
        b = bys.cpu().numpy()
        L = nchunks * 8
        idx = offs_np[:-1, None] + np.arange(L)[None, :]
        mask = np.arange(L)[None, :] < lens_np[:, None]
        padded = np.where(mask, b[np.minimum(idx, max(0, len(b) - 1))], 0)
        keys = padded.reshape(n, nchunks, 8).astype(np.uint64)
        shifts = np.uint64(8) * np.arange(7, -1, -1, dtype=np.uint64)
        words = (keys << shifts[None, None, :]).sum(axis=2, dtype=np.uint64)
        words ^= np.uint64(1 << 63)
        out = [torch.from_numpy(words[:, ci].view(np.int64).copy())
               for ci in range(nchunks)]
    out.append(lens)
    return out


def merge_key_order(
    file_pk_cols: List[List[Column]], counts: List[int], device
):
    """Return (order, sorted_keys_or_None, eq_tensors_or_None): global row
    order (indices into the concatenated rows) sorted by
    (pk..., file_seq, row) — the MOR merge order. When the PK packs into
    a u64 the merge-path kernel is used and the merged key array comes
    back for free (boundary detection reuses it, no re-gather). For other
    PKs (incl. strings) eq_tensors (concat space, most-significant-first)
    drive both the stable LSD sort and group-boundary detection."""
    per_file_keys = [_pack_keys_one_file(cols) for cols in file_pk_cols]
    if all(k is not None for k in per_file_keys) and len(per_file_keys) >= 1:
        # merge-path pairwise merge: order carries the global row index
        keys, order = hip().merge_sorted_keys(per_file_keys)
        return order, keys, None

    # generic stable LSD sort on concatenated keys (ties keep concat
    # order = snapshot order, the MOR tie rule)
    perm = torch.arange(sum(counts), dtype=torch.int64, device=device)
    sort_tensors: List[torch.Tensor] = []   # most-significant first
    npk = len(file_pk_cols[0])
    for ci in range(npk):
        cols = [fc[ci] for fc in file_pk_cols]
        if cols[0].is_string:
            sort_tensors.extend(_string_sort_tensors(cols, device))
        else:
            sort_tensors.append(torch.cat([c.data for c in cols]))
    for t in reversed(sort_tensors):
        k = t[perm]
        order = torch.argsort(k, stable=True)
        perm = perm[order]
    return perm, None, sort_tensors


def merge_sorted_files_gpu(
    file_batches: List[Batch],
    pk: List[str],
    merge_ops: Optional[Dict[str, str]] = None,
    cdc_column: Optional[str] = None,
    present: Optional[List[set]] = None,
) -> Batch:
    merge_ops = merge_ops or {}
    device = None
    for b in file_batches:
        for c in b.columns.values():
            t = c.data if not c.is_string else c.bytes_
            if t is not None:
                device = t.device
                break
        break
    schema = file_batches[0].schema
    names = schema.names()
    counts = [b.num_rows for b in file_batches]
    total = sum(counts)
    file_pk_cols = [[b.columns[p] for p in pk] for b in file_batches]

    order, sorted_keys, eq_tensors = merge_key_order(file_pk_cols, counts, device)

    # group boundaries: from the merged u64 keys when available (one
    # kernel), else from gathered pk values
    n = total
    if sorted_keys is not None:
        start = hip().group_start_mask(sorted_keys).to(torch.bool) if n else torch.zeros(0, dtype=torch.bool, device=device)
    else:
        start = torch.zeros(n, dtype=torch.bool, device=device)
        if n:
            start[0] = True
            for t in eq_tensors:
                sp = t[order]
                start[1:] |= sp[1:] != sp[:-1]
    # last row index (in sorted space) per group
    end_mask = torch.zeros(n, dtype=torch.bool, device=device)
    if n:
        end_mask[-1] = True
        end_mask[:-1] = start[1:]

    simple = all(merge_ops.get(nm, "UseLast") == "UseLast" for nm in names)
    uniform_cols = present is None or all(
        set(names) <= p for p in present
    )

    grp = seq_sorted = None
    ngroups = 0
    if not (simple and uniform_cols):
        # group ids + file seq per sorted row: only the merge-operator /
        # partial-column paths need them (one extra device sync)
        grp = torch.cumsum(start.to(torch.int64), 0) - 1
        ngroups = int(grp[-1].item()) + 1 if n else 0
        seq = torch.cat(
            [
                torch.full((c,), i, dtype=torch.int32, device=device)
                for i, c in enumerate(counts)
            ]
        ) if n else torch.empty(0, dtype=torch.int32, device=device)
        seq_sorted = seq[order]

    cat_cols: Dict[str, Column] = {}

    def cat_col(name: str) -> Column:
        if name not in cat_cols:
            from .batch import concat_batches

            cols = [b.columns[name] for b in file_batches]
            f = schema.field(name)
            cat_cols[name] = concat_batches(
                [Batch(Schema([f]), {name: c}) for c in cols]
            ).columns[name]
        return cat_cols[name]

    out_cols: Dict[str, Column] = {}
    if simple and uniform_cols:
        # UseLast for every column: survivors = last sorted row per group
        surv_sorted_idx = torch.nonzero(end_mask, as_tuple=True)[0]
        src_idx = order[surv_sorted_idx]
        out_cols = _gather_all(names, cat_col, src_idx)
    else:
        # per-column ops over group structure
        for name in names:
            op = merge_ops.get(name, "UseLast")
            if name in pk:
                op = "UseLast"
            col = cat_col(name)
            f = schema.field(name)
            contrib = None
            if present is not None:
                pres = torch.tensor(
                    [name in p for p in present], dtype=torch.uint8, device=device
                )
                if not bool(pres.all()):
                    contrib = pres[seq_sorted.to(torch.int64)]
            out_cols[name] = _apply_op_gpu(
                f, col, op, order, grp, ngroups, seq_sorted, start, end_mask, contrib
            )

    out_schema = schema
    out = Batch(out_schema, out_cols)

    if cdc_column and cdc_column in out.columns:
        c = out.columns[cdc_column]
        pattern = torch.frombuffer(bytearray(b"delete"), dtype=torch.uint8).to(device)
        keep = hip().bytes_ne_mask(c.offsets.to(torch.int64), c.bytes_, pattern)
        idx = torch.nonzero(keep.to(torch.bool), as_tuple=True)[0]
        out = out.take(idx)
    return out


def _gather_all(names, cat_col, src_idx) -> Dict[str, Column]:
    """Rows src_idx of every named column: fixed-width data and validity
    in fused multi-column gathers, strings through Column.take."""
    keys, tensors = [], []
    for name in names:
        c = cat_col(name)
        if c.is_string:
            continue
        keys.append((name, "data"))
        tensors.append(c.data)
        if c.validity is not None:
            keys.append((name, "validity"))
            tensors.append(c.validity)
    gathered = dict(zip(keys, hip().gather_fixed_multi(tensors, src_idx))) if tensors else {}
    out: Dict[str, Column] = {}
    for name in names:
        c = cat_col(name)
        if c.is_string:
            out[name] = c.take(src_idx)
        else:
            out[name] = Column(c.dtype, data=gathered[name, "data"],
                               validity=gathered.get((name, "validity")))
    return out


def _apply_op_gpu(f, col: Column, op: str, order, grp, ngroups, seq_sorted,
                  start, end_mask, contrib) -> Column:
    device = order.device
    n = order.numel()
    validity_sorted = (
        col.validity[order] if col.validity is not None else torch.empty(0, dtype=torch.uint8, device=device)
    )
    empty_u8 = torch.empty(0, dtype=torch.uint8, device=device)

    if op == "UseLast":
        if contrib is None:
            surv = torch.nonzero(end_mask, as_tuple=True)[0]
            src = order[surv]
            return _gather_one(f, col, src)
        last = hip().segmented_last(grp, contrib, empty_u8, ngroups, n)
        has = last >= 0
        src = order[torch.clamp(last, min=0)]
        res = _gather_one(f, col, src)
        base_v = res.validity if res.validity is not None else torch.ones(ngroups, dtype=torch.uint8, device=device)
        res.validity = (base_v.to(torch.bool) & has).to(torch.uint8)
        return res

    if op == "UseLastNotNull":
        vmask = validity_sorted if col.validity is not None else empty_u8
        cb = contrib if contrib is not None else empty_u8
        last = hip().segmented_last(grp, cb, vmask, ngroups, n)
        has = last >= 0
        src = order[torch.clamp(last, min=0)]
        res = _gather_one(f, col, src)
        res.validity = has.to(torch.uint8)
        return res

    if op in ("SumAll", "SumLast"):
        if col.is_string:
            raise TypeError("sum merge operator on string column")
        data_sorted = col.data[order]
        if data_sorted.dtype in (torch.int16, torch.int8):
            # the kernel sums int32 at the narrowest; .to(col.data.dtype)
            # below wraps to the column's width as the CPU merge does
            data_sorted = data_sorted.to(torch.int32)
        if op == "SumLast":
            los = torch.zeros(n, dtype=torch.bool, device=device)
            if n:
                los[-1] = True
                los[:-1] = (seq_sorted[1:] != seq_sorted[:-1]) | start[1:]
            base_contrib = los.to(torch.uint8)
            if contrib is not None:
                base_contrib = (base_contrib.to(torch.bool) & contrib.to(torch.bool)).to(torch.uint8)
        else:
            base_contrib = contrib if contrib is not None else empty_u8
        sums, has_null = hip().segmented_sum(
            data_sorted, grp, base_contrib, validity_sorted, ngroups
        )
        validity = (has_null == 0).to(torch.uint8)
        return Column(f.dtype, data=sums.to(col.data.dtype),
                      validity=None if bool(validity.all()) else validity)

    if op in ("JoinedAllByComma", "JoinedAllBySemicolon",
              "JoinedLastByComma", "JoinedLastBySemicolon"):
        # delimiter-join of (all | last-per-file) values per PK group.
        # Pure tensor algebra + the string gather kernel: participation
        # mask -> per-group ranks -> value byte layout with 1-byte gaps
        # for delimiters -> wave-per-row byte gather + delimiter scatter.
        delim = ord(",") if op.endswith("Comma") else ord(";")
        use_all = "All" in op
        participate = torch.ones(n, dtype=torch.bool, device=device)
        if contrib is not None:
            participate &= contrib.to(torch.bool)
        if not use_all:
            los = torch.zeros(n, dtype=torch.bool, device=device)
            if n:
                los[-1] = True
                los[:-1] = (seq_sorted[1:] != seq_sorted[:-1]) | start[1:]
            participate &= los
        # group is null if ANY participating row is null
        if col.validity is not None:
            null_part = participate & ~validity_sorted.to(torch.bool)
            gnull = torch.zeros(ngroups, dtype=torch.bool, device=device)
            gnull.index_put_((grp[null_part],),
                             torch.ones((), dtype=torch.bool, device=device))
        else:
            gnull = torch.zeros(ngroups, dtype=torch.bool, device=device)
        participate &= ~gnull[grp]

        offs = col.offsets.to(torch.int64).to(device)
        lens_all = offs[1:] - offs[:-1]
        lens_sorted = lens_all[order] * participate
        # rank of each participating row within its group (1-based)
        cp = torch.cumsum(participate.to(torch.int64), 0)
        gstarts = torch.nonzero(start, as_tuple=True)[0]
        base = torch.where(gstarts > 0, cp[gstarts - 1],
                           torch.zeros((), dtype=torch.int64, device=device))
        rank = cp - base[grp]
        has_delim = participate & (rank > 1)
        span = lens_sorted + has_delim.to(torch.int64)
        dst_end = torch.cumsum(span, 0)
        dst_start = dst_end - span
        total_bytes = int(dst_end[-1].item()) if n else 0
        # per-group output offsets from group-end cumulative bytes
        gends = torch.nonzero(end_mask, as_tuple=True)[0]
        out_offs = torch.zeros(ngroups + 1, dtype=torch.int64, device=device)
        if n:
            out_offs[1:] = dst_end[gends]
        sel = torch.nonzero(participate, as_tuple=True)[0]
        src_rows = order[sel]
        val_starts = dst_start[sel] + has_delim[sel].to(torch.int64)
        # dst_offsets arg needs n+1 entries; only starts are read (the
        # kernel uses source lengths) — append total as sentinel
        dstoffs = torch.cat([val_starts, torch.tensor([total_bytes], device=device)])
        out_bytes = hip().gather_strings(col.bytes_.to(device), offs, src_rows, dstoffs)
        dpos = dst_start[sel[has_delim[sel]]] if bool(has_delim.any()) else None
        if dpos is not None and dpos.numel():
            out_bytes.index_put_((dpos,), torch.tensor(
                delim, dtype=torch.uint8, device=device))
        validity = (~gnull).to(torch.uint8)
        return Column(col.dtype, None, out_offs, out_bytes,
                      None if bool(gnull.logical_not().all()) else validity)

    raise NotImplementedError(
        f"merge operator {op} not supported on GPU — scan with device='cpu'"
    )


def _gather_one(f, col: Column, src_idx) -> Column:
    return _gather_all([f.name], lambda _name: col, src_idx)[f.name]
