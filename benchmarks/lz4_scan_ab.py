"""The headline table of bench.py (same schema, value generators and bucket
count; sizes from the command line) written twice, as zstd and as lz4_raw,
and scanned merge-on-read on one GPU:

  zstd        the default codec, routes as configured
  lz4_gpu     LZ4_RAW pages decoded by csrc/hip/lz4.hip (LAKESOUL_GPU_LZ4=1)
  lz4_host    the same files, pages decoded by the host pool (=0)

The three are sampled in turn, ROUNDS times after one untimed round, so a
drift of the machine hits all of them; a sample is SCANS whole scans back
to back, reported as milliseconds per scan. Prints file bytes per codec,
every sample, and one JSON line with the fastest, median and slowest
of each. The last line says whether the GPU route's slowest scan beat the
host route's fastest: that decides the default of LAKESOUL_GPU_LZ4."""
import argparse, json, os, shutil, sys, tempfile, time

import numpy as np, torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

p = argparse.ArgumentParser()
p.add_argument("--rows-base", type=int, default=10_000_000)
p.add_argument("--rows-upsert", type=int, default=2_000_000)
p.add_argument("--upserts", type=int, default=10)
p.add_argument("--buckets", type=int, default=16)
p.add_argument("--rounds", type=int, default=5)
p.add_argument("--scans", type=int, default=5, help="scans per timed sample")
args = p.parse_args()
assert torch.cuda.is_available(), "needs a GPU"

workdir = tempfile.mkdtemp(prefix="lz4ab_")
os.environ["LAKESOUL_META_DB"] = os.path.join(workdir, "meta.db")
from lakesoul_amd.io import reader_gpu
from lakesoul_amd.io.schema import Field, Schema
from lakesoul_amd.meta.client import MetaClient
from lakesoul_amd.meta.store import SqliteMetaStore
from lakesoul_amd.tables.catalog import LakeSoulCatalog

catalog = LakeSoulCatalog(MetaClient(SqliteMetaStore(os.environ["LAKESOUL_META_DB"])),
                          warehouse=os.path.join(workdir, "wh"))
schema = Schema([Field("id", "int64", False), Field("v", "float64", False),
                 Field("k", "int32", False), Field("f", "float32", False),
                 Field("t", "int64", False)])


def gen(rng, ids):
    n = len(ids)
    return {"id": ids, "v": rng.normal(size=n),
            "k": rng.integers(0, 1000, n, dtype=np.int32),
            "f": rng.normal(size=n).astype(np.float32),
            "t": rng.integers(0, 10**12, n, dtype=np.int64)}


tables, file_bytes, write_s = {}, {}, {}
for codec in ("zstd", "lz4_raw"):
    t = catalog.create_table("ab_" + codec, schema, primary_keys=["id"],
                             hash_bucket_num=args.buckets,
                             properties={"compression": codec})
    rng = np.random.default_rng(1234)  # the same rows in both tables
    t0 = time.time()
    t.upsert(gen(rng, np.arange(args.rows_base, dtype=np.int64)), device="cuda")
    for _ in range(args.upserts):
        ids = rng.choice(args.rows_base, args.rows_upsert, replace=False).astype(np.int64)
        t.upsert(gen(rng, ids), device="cuda")
    write_s[codec] = round(time.time() - t0, 2)
    tables[codec] = t
    file_bytes[codec] = sum(os.path.getsize(f.path) for f in t.files())
print(json.dumps({"file_bytes": file_bytes, "write_s": write_s}), flush=True)


def scan_ms(table, gpu_lz4):
    reader_gpu._GPU_LZ4 = gpu_lz4
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.scans):
        rows = sum(b.num_rows for b in table.scan(device="cuda").iter_batches())
        assert rows == args.rows_base, rows
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / args.scans


arms = {"zstd": (tables["zstd"], True), "lz4_gpu": (tables["lz4_raw"], True),
        "lz4_host": (tables["lz4_raw"], False)}
ms = {k: [] for k in arms}
for r in range(args.rounds + 1):
    for name, (table, flag) in arms.items():
        v = scan_ms(table, flag)
        if r:  # round 0 warms the file and descriptor caches of every arm
            ms[name].append(round(v, 1))
print(json.dumps({"scan_ms": ms}), flush=True)
summary = {k: {"min": min(v), "median": float(np.median(v)), "max": max(v)}
           for k, v in ms.items()}
print(json.dumps({"rows": args.rows_base, "upserts": args.upserts,
                  "rows_upsert": args.rows_upsert, "summary_ms": summary,
                  "gpu_route_slowest_beats_host_fastest":
                      summary["lz4_gpu"]["max"] < summary["lz4_host"]["min"]}),
      flush=True)
shutil.rmtree(workdir, ignore_errors=True)
