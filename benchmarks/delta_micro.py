"""DELTA_BINARY_PACKED / BYTE_STREAM_SPLIT unit read: GPU route (raw pages
over the bus, delta.hip decode) against host route (host decode, 8 B/row
over the bus) on the same pyarrow-written file. One unit = one file; the
timed section is read_unit_raw + H2D + decode_unit + device sync, the path
a GPU scan takes per unit. Prints one JSON line per column kind and route
with GB/s of DECODED output (median of --reps after one warm-up).

    python benchmarks/delta_micro.py [--rows 8000000] [--reps 7]
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
kinds = {
    "i64_sorted_key": (np.cumsum(rng.integers(1, 16, n)).astype(np.int64), "DELTA_BINARY_PACKED"),
    "i64_timestamp": ((1_700_000_000_000_000 + np.cumsum(rng.integers(0, 2_000_000, n))).astype(np.int64), "DELTA_BINARY_PACKED"),
    "i64_random": (rng.integers(-2**62, 2**62, n).astype(np.int64), "DELTA_BINARY_PACKED"),
    "f64_normal": (rng.normal(size=n), "BYTE_STREAM_SPLIT"),
}
e_u8 = torch.empty(0, dtype=torch.uint8, device=dev)
e_i64 = torch.empty(0, dtype=torch.int64, device=dev)


def once(path, gpu_route):
    t0 = time.perf_counter()
    raw = cpp().read_unit_raw([path], ["x"], 0, True, False, False, 1.0, gpu_route)
    t1 = time.perf_counter()
    tr = UnitTransfer(raw, dev)
    outs = hip().decode_unit(tr.vals, e_u8, e_u8, e_i64, e_i64, raw["desc"], 1, 1, tr.enc)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, raw["values"].numel(), outs[0][0]


with tempfile.TemporaryDirectory() as td:
    for name, (vals, enc) in kinds.items():
        path = os.path.join(td, name + ".parquet")
        pq.write_table(pa.table({"x": pa.array(vals)}), path, use_dictionary=False,
                       column_encoding={"x": enc}, compression="zstd",
                       row_group_size=1 << 20)
        want = torch.from_numpy(vals.view(np.int64))
        for route, flag in (("gpu", True), ("host", False)):
            _, _, shipped, out = once(path, flag)  # warm-up + correctness
            assert torch.equal(out.view(torch.int64).cpu(), want), (name, route)
            host, devt = [], []
            for _ in range(args.reps):
                h, d, _, _ = once(path, flag)
                host.append(h)
                devt.append(d)
            total = float(np.median(np.array(host) + np.array(devt)))
            print(json.dumps({
                "kind": name, "encoding": enc, "route": route, "rows": n,
                "file_mb": round(os.path.getsize(path) / 1e6, 1),
                "h2d_mb": round(shipped / 1e6, 1),
                "host_ms": round(float(np.median(host)) * 1e3, 2),
                "h2d_decode_ms": round(float(np.median(devt)) * 1e3, 2),
                "decoded_gbps": round(n * 8 / total / 1e9, 2)}), flush=True)
