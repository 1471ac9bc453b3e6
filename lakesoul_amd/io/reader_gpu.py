"""GPU read path: host IO/decompress -> single H2D -> HIP decode -> GPU merge.

Pipeline per scan unit:
1. host (C++ thread pool, one call per unit): footer parse, page walk,
   zstd/snappy decompress, def-level RLE decode, and layout of every
   chunk payload into a handful of contiguous (pinned) buffers
   (_cpp.read_unit_raw / csrc/cpp/read_unit.h);
2. ONE async H2D per buffer (values / validity / dicts / runs / enc);
3. HIP kernels materialize columns in HBM: PLAIN fixed-width columns are
   zero-copy views into the device buffer; dictionary chunks expand with
   the RLE bit-unpack kernel + fused dict-gather/null-scatter; raw
   DELTA_BINARY_PACKED / BYTE_STREAM_SPLIT pages decode with the delta.hip
   kernels; nullable PLAIN columns scatter through validity;
4. GPU merge-on-read (merge_gpu) with the merge-path kernel.

String columns whose chunks in a file are all PLAIN or all dictionary-coded
ship raw: the host only walks the length prefixes (PLAIN) or the dictionary
page (dictionary), and csrc/hip/strings.hip moves the bytes in HBM, a
byte-parallel segment copy (read_unit.h, UD_STR). Mixed columns, lists and
nested leaves, and every string column under LAKESOUL_GPU_STRINGS=0, are
host-assembled ((len,bytes) stream is serial) and ship as (offsets int64,
bytes). The decoded (offsets, bytes, validity) triple is the same on both
routes.
"""

from __future__ import annotations

import os as _os
from typing import Dict, List, Optional

import numpy as np
import torch

from ..ops import cpp, hip
from ..utils import timing
from .batch import (Batch, Column, concat_batches, torch_dtype_for,
                    torch_phys_dtype_for)
from .merge_gpu import merge_sorted_files_gpu
from .schema import Field, Schema


def _host_threads_per_rank() -> int:
    try:
        quota_s = open("/sys/fs/cgroup/cpu.max").read().split()
        ncpu = _os.cpu_count() or 16
        quota = ncpu if quota_s[0] == "max" else max(
            1, int(quota_s[0]) // int(quota_s[1]))
    except OSError:
        quota = _os.cpu_count() or 16
    world = int(_os.environ.get("WORLD_SIZE", "1"))
    return max(1, quota // max(1, world))


def _default_gpu_zstd_frac() -> float:
    """Fraction of zstd chunks decoded by the GPU kernel (the rest go to
    the host pool; the prefetch pipeline overlaps the two across units).

    Balanced split from measured single-source rates (profiles/
    r01_gpu_zstd.md: host pool ~90 ms/step at 16 threads, GPU v2 kernel
    ~136 ms/step): frac = host_rate/(host_rate+gpu_rate) scaled by the
    rank's actual thread budget. Starved ranks (<3 threads) go full GPU;
    LAKESOUL_GPU_ZSTD=0/1 still forces pure host / pure GPU and
    LAKESOUL_GPU_ZSTD_FRAC pins an explicit split."""
    env = _os.environ.get("LAKESOUL_GPU_ZSTD")
    if env is not None and env != "":
        if env == "0":
            return 0.0
        if env == "1":
            return 1.0
    envf = _os.environ.get("LAKESOUL_GPU_ZSTD_FRAC")
    if envf:
        return min(1.0, max(0.0, float(envf)))
    threads = _host_threads_per_rank()
    # Measured r2 A/B on the headline bench (gpurun bench_frac_*.log):
    # host-only 40 ms/step, frac=0.4 342 ms, frac=1.0 371 ms at the
    # 128 KB default pages — the GPU kernel's wave-per-page parallelism
    # collapses on large pages (it wants thousands of 32 KB pages per
    # unit, profiles/r01_gpu_zstd.md). Hybrid stays opt-in via
    # LAKESOUL_GPU_ZSTD_FRAC (+ LAKESOUL_PAGE_BYTES=32768 at write time);
    # the adaptive rule keeps full-GPU decode for starved ranks only.
    if threads < 6:
        return 1.0
    return 0.0


_GPU_ZSTD_FRAC = _default_gpu_zstd_frac()
_GPU_ZSTD = _GPU_ZSTD_FRAC > 0.0

# DELTA_BINARY_PACKED / BYTE_STREAM_SPLIT pages of foreign files: ship the
# raw pages and decode them in HBM (csrc/hip/delta.hip) unless
# LAKESOUL_GPU_DELTA=0 forces the host decode. The default rests on bus
# volume (a delta-packed sorted int64 key is a few bits per row against
# 8 B/row host-decoded) and on one micro-benchmark of single-column unit
# reads (benchmarks/delta_micro.py, profiles/delta_micro.md: GPU route
# 1.4x-7x the host route); no scan-level A/B has been measured.
_GPU_DELTA = _os.environ.get("LAKESOUL_GPU_DELTA", "1") != "0"

# Huffman-only zstd pages (one compressed block, Huffman literals, no
# sequences: float columns, wide-range integers) decode on the GPU, 256
# lanes per Huffman stream (csrc/hip/zstd_huf.hip), and leave the host pool;
# the unit's other pages follow LAKESOUL_GPU_ZSTD* as before.
# LAKESOUL_GPU_HUF=0 sends them back to where they went without it.
# Measured: profiles/r03_gpu_huf.md.
_GPU_HUF = _os.environ.get("LAKESOUL_GPU_HUF", "1") != "0"

# LZ4_RAW pages of REQUIRED fixed-width PLAIN columns: the host pool decodes
# them straight into the values buffer, as it does zstd pages.
# LAKESOUL_GPU_LZ4=1 sends them to the GPU instead, one wave per page
# (csrc/hip/lz4.hip): their compressed bytes cross the bus and the host
# never touches them. Off by default: on the headline table the GPU route
# scans in 252 ms against 28 ms (the kernel walks a page's sequences
# serially, about 1 us each, and a scan unit holds only a few hundred
# pages). Measured: profiles/r04_gpu_lz4.md.
_GPU_LZ4 = _os.environ.get("LAKESOUL_GPU_LZ4", "0") == "1"

# GZIP pages of REQUIRED fixed-width PLAIN columns: the host pool inflates
# them straight into the values buffer (csrc/cpp/inflate.h), as it does
# zstd pages. LAKESOUL_GPU_GZIP=1 sends them to the GPU instead, one wave
# per page (csrc/hip/gzip.hip); that route checks framing, ISIZE and the
# output length but not CRC32. Off by default: on a pyarrow-written GZIP
# copy of the headline table the GPU route scans in 575 ms against 217 ms
# (a wave decodes a page's symbols one by one, and a scan unit holds only a
# few hundred pages). Measured: profiles/r08_gpu_gzip.md.
_GPU_GZIP = _os.environ.get("LAKESOUL_GPU_GZIP", "0") == "1"


# String columns whose chunks are all PLAIN (or all dictionary-encoded):
# ship the raw streams and let the GPU strip the prefixes / expand the
# dictionary (csrc/hip/strings.hip) instead of assembling the bytes on the
# host. Mixed columns, lists and nested leaves stay host-assembled.
# On by default for both kinds; LAKESOUL_GPU_STRINGS=0 forces the host
# route. Measured on single-column unit reads (benchmarks/string_micro.py,
# profiles/r05_gpu_strings.md): a 7-value dictionary column of 8 M rows
# 159 ms -> 2.4 ms (3.8 MB over the bus instead of 103 MB), 40-byte PLAIN
# keys 424 ms -> 130 ms, 1 KB PLAIN values 1351 ms -> 805 ms, each gap
# larger than the run-to-run spread; the headline scan (no string column)
# is unchanged.
_GPU_STRINGS = _os.environ.get("LAKESOUL_GPU_STRINGS", "1") != "0"


def fetch_raw(files: List[str], names: List[str]) -> dict:
    """Host phase of a unit read (releases the GIL in C++) — safe to run
    on a prefetch thread while the GPU processes the previous unit."""
    with timing.phase("host_fetch"):
        raw = cpp().read_unit_raw(files, names, 0, True, True, _GPU_ZSTD,
                                  _GPU_ZSTD_FRAC, _GPU_DELTA, _GPU_HUF,
                                  _GPU_LZ4, _GPU_STRINGS, _GPU_GZIP)
    if timing.ENABLED:
        timing._acc["fetch.stage1"] += raw["t_stage1_us"] / 1e6
        timing._acc["fetch.s1_open"] += raw["t_open_us"] / 1e6
        timing._acc["fetch.s1_chunks"] += raw["t_chunks_us"] / 1e6
        timing._acc["fetch.s1_layout"] += raw["t_layout_us"] / 1e6
        timing._acc["fetch.alloc"] += raw["t_alloc_us"] / 1e6
        timing._acc["fetch.fill"] += raw["t_fill_us"] / 1e6
        timing._cnt["fetch.stage1"] += 1
    return raw


class UnitTransfer:
    """Async H2D of one unit's buffers (default stream: the python thread
    runs ahead of the GPU, so next-unit copies already pipeline behind
    the current unit's kernels; a dedicated copy stream measured ~8%
    SLOWER from event/ordering overhead — kept default)."""

    def __init__(self, raw: dict, device):
        self.raw = raw  # hold pinned host buffers until consumed
        # values regions covered by GPU decompress jobs carry no host
        # data — ship only the host-filled gaps (for all-zstd units the
        # H2D volume drops to the compressed bytes)
        jobs_host = []
        for k in ("snappy_jobs", "zstd_jobs", "huf_jobs", "lz4_jobs", "gzip_jobs"):
            t = raw.get(k)
            if t is not None and t.numel():
                jobs_host.append(t.view(-1, 4))
        nvals = raw["values"].numel()
        if jobs_host and nvals:
            j = torch.cat(jobs_host) if len(jobs_host) > 1 else jobs_host[0]
            dst = j[:, 2].numpy()
            ln = j[:, 3].numpy()
            order = dst.argsort()
            dst, ln = dst[order], ln[order]
            ends = np.maximum.accumulate(dst + ln)
            gap_starts = np.concatenate(([0], ends))
            gap_ends = np.concatenate((dst, [nvals]))
            keep = gap_ends > gap_starts
            self.vals = torch.empty(nvals, dtype=torch.uint8, device=device)
            gaps = np.stack((gap_starts[keep], gap_ends[keep]), axis=1)
            hip().copy_ranges_h2d(raw["values"], self.vals,
                                  torch.from_numpy(gaps.astype(np.int64)))
        else:
            self.vals = raw["values"].to(device, non_blocking=True)
        self.validity = (
            raw["validity"].to(device, non_blocking=True)
            if raw["validity"].numel() else None
        )
        self.dicts = raw["dicts"].to(device, non_blocking=True) if raw["dicts"].numel() else None
        self.runs = (
            raw["runs"].view(-1, 6).to(device, non_blocking=True)
            if raw["runs"].numel() else None
        )
        self.soffs = raw["soffs"].to(device, non_blocking=True) if raw["soffs"].numel() else None
        self.enc = (
            raw["enc"].view(-1, 6).to(device, non_blocking=True)
            if raw.get("enc") is not None and raw["enc"].numel() else None
        )
        self.comp = raw["comp"].to(device, non_blocking=True) if raw.get("comp") is not None and raw["comp"].numel() else None
        self.snappy_jobs = (
            raw["snappy_jobs"].view(-1, 4).to(device, non_blocking=True)
            if raw.get("snappy_jobs") is not None and raw["snappy_jobs"].numel()
            else None
        )
        self.zstd_jobs = (
            raw["zstd_jobs"].view(-1, 4).to(device, non_blocking=True)
            if raw.get("zstd_jobs") is not None and raw["zstd_jobs"].numel()
            else None
        )
        self.huf_jobs = (
            raw["huf_jobs"].view(-1, 4).to(device, non_blocking=True)
            if raw.get("huf_jobs") is not None and raw["huf_jobs"].numel()
            else None
        )
        self.lz4_jobs = (
            raw["lz4_jobs"].view(-1, 4).to(device, non_blocking=True)
            if raw.get("lz4_jobs") is not None and raw["lz4_jobs"].numel()
            else None
        )
        self.gzip_jobs = (
            raw["gzip_jobs"].view(-1, 4).to(device, non_blocking=True)
            if raw.get("gzip_jobs") is not None and raw["gzip_jobs"].numel()
            else None
        )


def _check_huf_status(status) -> None:
    """Raise if the Huffman kernel refused a page. Called once the unit's
    decode has synchronized anyway: no host sync of its own per unit."""
    if status is not None and bool((status != 0).any()):
        raise RuntimeError(
            f"GPU zstd Huffman decode failed: status={int((status != 0).sum())} pages")


def _wrap_column(f, entry) -> Column:
    """One decoded entry of _hip.decode_unit / scan_unit_uselast as a
    Column of the unit's work schema."""
    if f.dtype.startswith("list<"):
        # list<T> columns travel the unit as BYTE-offset binary (element
        # payload in the string-bytes region) so the merge machinery treats
        # whole lists opaquely (UseLast whole-value, merge/mod.rs:65-89);
        # converted back to element-offset list columns by the projection
        offs, by, vmask = entry
        es = torch_phys_dtype_for(f.dtype[5:-1]).itemsize
        return Column("binary", offsets=offs * es, bytes_=by, validity=vmask)
    if f.dtype in ("string", "binary"):
        offs, by, vmask = entry
        return Column(f.dtype, offsets=offs, bytes_=by, validity=vmask)
    data, vmask = entry
    data = data.view(torch_phys_dtype_for(f.dtype))
    if data.dtype != torch_dtype_for(f.dtype):
        # int8/int16: physical INT32, narrowed after decode
        data = data.to(torch_dtype_for(f.dtype))
    return Column(f.dtype, data=data, validity=vmask)


def _null_column(f, nrows, device) -> Column:
    """All-null column for a file that lacks the field (schema evolution)."""
    validity = torch.zeros(nrows, dtype=torch.uint8, device=device)
    if f.dtype in ("string", "binary") or f.dtype.startswith("list<"):
        return Column(
            "binary" if f.dtype.startswith("list<") else f.dtype,
            offsets=torch.zeros(nrows + 1, dtype=torch.int64, device=device),
            bytes_=torch.empty(0, dtype=torch.uint8, device=device),
            validity=validity)
    return Column(
        f.dtype,
        data=torch.zeros(nrows, dtype=torch_dtype_for(f.dtype), device=device),
        validity=validity)


def read_unit_gpu(scan, unit, raw: Optional[dict] = None) -> Optional[Batch]:
    device = torch.device("cuda")
    names = scan.read_cols
    if raw is None:
        raw = fetch_raw(unit.files, names)
    with timing.phase("h2d"):
        transfer = UnitTransfer(raw, device)
    vals = transfer.vals
    if transfer.snappy_jobs is not None:
        # GPU snappy: decompress page bodies straight into the values
        # buffer (wave-per-page kernel) — no host decompression happened
        # for these chunks
        status = hip().snappy_decompress_into(transfer.comp, transfer.snappy_jobs, vals)
        if bool((status != 0).any()):
            raise RuntimeError(f"GPU snappy decompression failed: {status.cpu().tolist()}")
    if transfer.lz4_jobs is not None:
        # GPU LZ4: LZ4_RAW page blocks straight into the values buffer
        status = hip().lz4_decompress_into(transfer.comp, transfer.lz4_jobs, vals)
        if bool((status != 0).any()):
            raise RuntimeError(f"GPU lz4 decompression failed: status={int((status != 0).sum())} pages")
    if transfer.gzip_jobs is not None:
        # GPU GZIP: GZIP pages straight into the values buffer
        status = hip().gzip_decompress_into(transfer.comp, transfer.gzip_jobs, vals)
        if bool((status != 0).any()):
            raise RuntimeError(f"GPU gzip decompression failed: status={int((status != 0).sum())} pages")
    if transfer.zstd_jobs is not None:
        # GPU zstd: the from-scratch RFC 8878 decoder (csrc/hip/zstd.hip)
        # decompresses zstd page frames straight into the values buffer —
        # compressed bytes crossed the bus, the cgroup-capped host CPUs
        # never touched them
        status = hip().zstd_decompress_into(transfer.comp, transfer.zstd_jobs, vals)
        if bool((status != 0).any()):
            raise RuntimeError(f"GPU zstd decompression failed: status={int((status != 0).sum())} pages")
    huf_status = None
    if transfer.huf_jobs is not None:
        # Huffman-only zstd pages: a workgroup per page, straight into the
        # values buffer; the status is read after the unit's decode
        huf_status = hip().zstd_huf_decompress_into(transfer.comp, transfer.huf_jobs, vals)

    fields = [scan._field_for(n) for n in names]
    has_list = any(f.dtype.startswith("list<") for f in fields)
    # list<T> leaves are binary lanes until the projection (_wrap_column)
    work_schema = Schema([
        Field(f.name, "binary" if f.dtype.startswith("list<") else f.dtype,
              f.nullable)
        for f in fields])
    ncols = len(names)
    nfiles = len(raw["file_rows"])
    desc = raw["desc"]
    empty_u8 = torch.empty(0, dtype=torch.uint8, device=device)
    empty_i64 = torch.empty(0, dtype=torch.int64, device=device)
    unit_bufs = (
        vals,
        transfer.validity if transfer.validity is not None else empty_u8,
        transfer.dicts if transfer.dicts is not None else empty_u8,
        transfer.runs if transfer.runs is not None else empty_i64,
        transfer.soffs if transfer.soffs is not None else empty_i64,
        desc, nfiles, ncols,
    )

    # ---- C++ fast path: decode + UseLast merge + gather in ONE call ----
    # (the per-unit python op storm was the scan's critical path)
    if (
        not has_list
        and nfiles > 1
        and len(scan.pk) == 1
        and not scan.merge_ops
        and scan.cdc_column is None
        and scan.pk[0] in names
        and scan.schema.field(scan.pk[0]).dtype in ("int64", "int32")
        and bool(desc[:, cpp().UD_PRESENT].all())
    ):
        with timing.phase("gpu_unit_cpp", sync_gpu=False):
            pk_ci = names.index(scan.pk[0])
            pk_es = 8 if scan.schema.field(scan.pk[0]).dtype == "int64" else 4
            outs = hip().scan_unit_uselast(*unit_bufs, pk_ci, pk_es,
                                           transfer.enc)
        _check_huf_status(huf_status)
        merged = {f.name: _wrap_column(f, outs[ci])
                  for ci, f in enumerate(fields)}
        return scan._to_eval_batch(merged, unit, len(merged[names[0]]), device)

    # ---- generic path: shared decode, python-driven merge ----
    file_batches: List[Batch] = []
    present: List[set] = []
    with timing.phase("gpu_decode", sync_gpu=True):
        outs = hip().decode_unit(*unit_bufs, transfer.enc)
        _check_huf_status(huf_status)
        for fi, nrows in enumerate(raw["file_rows"]):
            cols: Dict[str, Column] = {}
            pres = set()
            for ci, f in enumerate(fields):
                entry = outs[fi * ncols + ci]
                if entry is None:
                    cols[f.name] = _null_column(f, nrows, device)
                else:
                    pres.add(f.name)
                    cols[f.name] = _wrap_column(f, entry)
            file_batches.append(Batch(work_schema, cols))
            present.append(pres)

    if scan._needs_merge(nfiles):
        with timing.phase("gpu_merge", sync_gpu=True):
            merged = merge_sorted_files_gpu(
                file_batches, scan.pk, scan.merge_ops, scan.cdc_column, present
            )
    else:
        merged = concat_batches(file_batches)

    # project to eval schema (+ materialize range-partition columns);
    # filter-only columns are dropped after filter evaluation
    return scan._to_eval_batch(merged.columns, unit, merged.num_rows, device)
