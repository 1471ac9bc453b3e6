"""String column unit read: GPU route (the host walks the length prefixes or
the dictionary page, strings.hip moves the bytes) against host route (the
host assembles offsets and bytes) on the same pyarrow-written file. One unit
= one single-column file; the timed section is read_unit_raw + H2D +
decode_unit + device sync, the path a GPU scan takes per unit. The two
routes alternate within one process; per kind and route one JSON line with
the median, min and max of --reps repetitions after a warm-up, and the bytes
shipped over the bus (sum of the unit's buffer sizes). A last line per kind
says whether the GPU route wins by more than the larger max-min spread of
the two routes.

    python benchmarks/string_micro.py [--rows 8000000] [--reps 7]
"""
import argparse, json, os, sys, tempfile, time

import numpy as np, pyarrow as pa, pyarrow.parquet as pq, torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lakesoul_amd.io.reader_gpu import UnitTransfer
from lakesoul_amd.ops import cpp, hip

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=8_000_000)
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
n = args.rows
rng = np.random.default_rng(0)
dev = torch.device("cuda:0")


def string_array(lengths, blob):
    offs = np.zeros(len(lengths) + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lengths)
    return pa.LargeStringArray.from_buffers(
        len(lengths), pa.py_buffer(offs), pa.py_buffer(blob)).cast(pa.string())


def dict7(rows):
    """7 distinct values of up to 10 bytes (TPC-H ship modes)."""
    modes = ["AIR", "R", "TRUCK", "MAIL", "SHIP", "REG AIR", "FOB-EXPORT"]
    return pa.array(modes).take(pa.array(rng.integers(0, 7, rows)))


def keys40(rows):
    """Keys of 36..44 bytes: a shared prefix and the row number."""
    width = 44
    m = np.empty((rows, width), dtype=np.uint8)
    prefix = np.frombuffer(b"tenant-0001/region-eu-west/key-", dtype=np.uint8)
    m[:, :len(prefix)] = prefix
    i = np.arange(rows, dtype=np.int64)
    for d in range(width - len(prefix)):
        m[:, width - 1 - d] = 48 + (i // 10 ** d) % 10
    lengths = 36 + (i * 5) % 9
    blob = m[np.arange(width)[None, :] < lengths[:, None]]
    return string_array(lengths, blob)


def values1k(rows):
    """Values of 1000..1048 random lower-case bytes."""
    lengths = 1000 + (np.arange(rows, dtype=np.int64) * 11) % 49
    return string_array(lengths, rng.integers(97, 123, int(lengths.sum()), dtype=np.uint8))


kinds = {
    "dict7": (lambda: dict7(n), True),
    "plain_key40": (lambda: keys40(n), False),
    "plain_value1k": (lambda: values1k(max(n // 8, 1)), False),
}
e_u8 = torch.empty(0, dtype=torch.uint8, device=dev)
e_i64 = torch.empty(0, dtype=torch.int64, device=dev)
BUFS = ("values", "validity", "dicts", "runs", "soffs")


def once(path, gpu_route):
    t0 = time.perf_counter()
    raw = cpp().read_unit_raw([path], ["x"], 0, True, gpu_strings=gpu_route)
    t1 = time.perf_counter()
    tr = UnitTransfer(raw, dev)
    outs = hip().decode_unit(
        tr.vals, e_u8, tr.dicts if tr.dicts is not None else e_u8,
        tr.runs if tr.runs is not None else e_i64,
        tr.soffs if tr.soffs is not None else e_i64, raw["desc"], 1, 1, tr.enc)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    shipped = sum(raw[k].numel() * raw[k].element_size() for k in BUFS)
    return t1 - t0, t2 - t1, shipped, int(raw["desc"][0, cpp().UD_STR]), outs[0]


with tempfile.TemporaryDirectory() as td:
    for name, (make, use_dict) in kinds.items():
        arr = make()
        rows = len(arr)
        path = os.path.join(td, name + ".parquet")
        pq.write_table(pa.table({"x": arr}), path, use_dictionary=use_dict,
                       compression="zstd", row_group_size=1 << 20)
        del arr
        # warm-up and correctness: the two routes give the same column
        _, _, ship_g, tag, out_g = once(path, True)
        _, _, ship_h, tag_h, out_h = once(path, False)
        assert tag == (cpp().UD_STR_DICT if use_dict else cpp().UD_STR_PLAIN) and tag_h == 0
        assert torch.equal(out_g[0], out_h[0]) and torch.equal(out_g[1], out_h[1])
        out_bytes = out_g[1].numel()
        del out_g, out_h
        t = {"gpu": [], "host": []}
        h = {"gpu": [], "host": []}
        for _ in range(args.reps):  # the routes alternate
            for route, flag in (("host", False), ("gpu", True)):
                a, b, _, _, _ = once(path, flag)
                t[route].append(a + b)
                h[route].append(a)
        res = {}
        for route, shipped in (("host", ship_h), ("gpu", ship_g)):
            ms = np.array(t[route]) * 1e3
            res[route] = (float(np.median(ms)), float(ms.max() - ms.min()))
            print(json.dumps({
                "kind": name, "route": route, "rows": rows,
                "file_mb": round(os.path.getsize(path) / 1e6, 1),
                "string_mb": round(out_bytes / 1e6, 1),
                "shipped_mb": round(shipped / 1e6, 1),
                "host_fetch_ms": round(float(np.median(h[route])) * 1e3, 2),
                "median_ms": round(res[route][0], 2),
                "min_ms": round(float(ms.min()), 2),
                "max_ms": round(float(ms.max()), 2)}), flush=True)
        spread = max(res["host"][1], res["gpu"][1])
        print(json.dumps({
            "kind": name, "host_minus_gpu_ms": round(res["host"][0] - res["gpu"][0], 2),
            "spread_ms": round(spread, 2),
            "gpu_wins": bool(res["host"][0] - res["gpu"][0] > spread)}), flush=True)
