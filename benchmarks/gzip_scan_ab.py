"""The headline table of bench.py (same schema, value generators and bucket
count; sizes from the command line) written by the project as zstd, then
copied file by file with pyarrow as GZIP (PLAIN pages, --page-size bytes,
zlib level --level), and scanned merge-on-read on one GPU:

  zstd        the default codec, routes as configured
  gzip_host   the GZIP copy, pages inflated by the host pool
              (LAKESOUL_GPU_GZIP=0, csrc/cpp/inflate.h)
  gzip_gpu    the same files, pages inflated by csrc/hip/gzip.hip (=1)

Every sample is a fresh process (the reader takes the flag from the
environment at import): one untimed scan, then --scans scans back to back,
reported as milliseconds per scan. The arms are sampled in turn, --rounds
times, so a drift of the machine hits all of them. Prints file bytes per
codec, every sample, and one JSON line with the fastest, median and slowest
of each. The last field says whether the GPU route's slowest sample beat
the host route's fastest: that decides the default of LAKESOUL_GPU_GZIP."""
import argparse, json, os, shutil, subprocess, sys, tempfile, time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

p = argparse.ArgumentParser()
p.add_argument("--rows-base", type=int, default=10_000_000)
p.add_argument("--rows-upsert", type=int, default=2_000_000)
p.add_argument("--upserts", type=int, default=10)
p.add_argument("--buckets", type=int, default=16)
p.add_argument("--rounds", type=int, default=5)
p.add_argument("--scans", type=int, default=5, help="scans per timed sample")
p.add_argument("--page-size", type=int, default=128 << 10)
p.add_argument("--level", type=int, default=6)
p.add_argument("--child", nargs=3, metavar=("WORKDIR", "TABLE", "ROWS"),
               help="internal: one sample of TABLE in this process")
args = p.parse_args()


def open_catalog(workdir):
    from lakesoul_amd.meta.client import MetaClient
    from lakesoul_amd.meta.store import SqliteMetaStore
    from lakesoul_amd.tables.catalog import LakeSoulCatalog

    return LakeSoulCatalog(MetaClient(SqliteMetaStore(os.path.join(workdir, "meta.db"))),
                           warehouse=os.path.join(workdir, "wh"))


def child(workdir, name, rows):
    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    table = open_catalog(workdir).table(name)

    def scan():
        got = sum(b.num_rows for b in table.scan(device="cuda").iter_batches())
        assert got == int(rows), got

    scan()  # warms the file and descriptor caches
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.scans):
        scan()
    torch.cuda.synchronize()
    print(json.dumps({"ms": (time.perf_counter() - t0) * 1e3 / args.scans}), flush=True)


if args.child:
    child(*args.child)
    sys.exit(0)

import pyarrow.parquet as pq
import torch

assert torch.cuda.is_available(), "needs a GPU"
workdir = tempfile.mkdtemp(prefix="gzipab_")
from lakesoul_amd.io.schema import Field, Schema
from lakesoul_amd.meta.entities import CommitOp, DataCommitInfo, DataFileOp, FileOp

catalog = open_catalog(workdir)
schema = Schema([Field("id", "int64", False), Field("v", "float64", False),
                 Field("k", "int32", False), Field("f", "float32", False),
                 Field("t", "int64", False)])


def gen(rng, ids):
    n = len(ids)
    return {"id": ids, "v": rng.normal(size=n),
            "k": rng.integers(0, 1000, n, dtype=np.int32),
            "f": rng.normal(size=n).astype(np.float32),
            "t": rng.integers(0, 10**12, n, dtype=np.int64)}


kw = dict(primary_keys=["id"], hash_bucket_num=args.buckets)
tz = catalog.create_table("ab_zstd", schema, **kw)
rng = np.random.default_rng(1234)
t0 = time.time()
tz.upsert(gen(rng, np.arange(args.rows_base, dtype=np.int64)), device="cuda")
for _ in range(args.upserts):
    ids = rng.choice(args.rows_base, args.rows_upsert, replace=False).astype(np.int64)
    tz.upsert(gen(rng, ids), device="cuda")
write_s = round(time.time() - t0, 2)

# the GZIP copy: every file under its own name (the name carries the hash
# bucket), committed in the order of the original's commits
tg = catalog.create_table("ab_gzip", schema, **kw)
files = [(desc, f) for desc in tz.client.all_partition_descs(tz.table_id)
         for f in tz.files(desc)]


def copy(item):
    desc, f = item
    dst = os.path.join(tg.table_path, os.path.basename(f.path))
    pq.write_table(pq.read_table(f.path), dst, compression="gzip",
                   compression_level=args.level, use_dictionary=False,
                   data_page_size=args.page_size, write_statistics=False)
    return desc, dst


t0 = time.time()
with ThreadPoolExecutor(16) as pool:
    copies = list(pool.map(copy, files))
copy_s = round(time.time() - t0, 2)
for desc, dst in copies:
    tg.client.commit_data_commit_info(DataCommitInfo(
        table_id=tg.table_id, partition_desc=desc,
        file_ops=[DataFileOp(dst, FileOp.add, os.path.getsize(dst))],
        commit_op=CommitOp.MergeCommit))
file_bytes = {"zstd": sum(os.path.getsize(f.path) for _, f in files),
              "gzip": sum(os.path.getsize(d) for _, d in copies)}
md = pq.ParquetFile(copies[0][1]).metadata
assert md.row_group(0).column(0).compression == "GZIP"
print(json.dumps({"file_bytes": file_bytes, "files": len(files), "write_s": write_s,
                  "gzip_copy_s": copy_s}), flush=True)

# both tables hold the same merged rows
a = tz.scan(device="cuda").to_arrow().sort_by("id")
b = tg.scan(device="cuda").to_arrow().sort_by("id")
assert a.equals(b), "the GZIP copy does not merge to the original's rows"
del a, b


def sample(name, flag):
    env = dict(os.environ, LAKESOUL_GPU_GZIP=flag)
    r = subprocess.run(
        [sys.executable, os.path.abspath(__file__), "--scans", str(args.scans),
         "--child", workdir, name, str(args.rows_base)],
        env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])["ms"]


arms = {"zstd": ("ab_zstd", "0"), "gzip_host": ("ab_gzip", "0"),
        "gzip_gpu": ("ab_gzip", "1")}
ms = {k: [] for k in arms}
for r in range(args.rounds):
    for name, (table, flag) in arms.items():
        ms[name].append(round(sample(table, flag), 1))
    print(json.dumps({"round": r, "scan_ms": {k: v[-1] for k, v in ms.items()}}),
          flush=True)
summary = {k: {"min": min(v), "median": float(np.median(v)), "max": max(v)}
           for k, v in ms.items()}
print(json.dumps({"rows": args.rows_base, "upserts": args.upserts,
                  "rows_upsert": args.rows_upsert, "page_size": args.page_size,
                  "level": args.level, "scan_ms": ms, "summary_ms": summary,
                  "gpu_route_slowest_beats_host_fastest":
                      summary["gzip_gpu"]["max"] < summary["gzip_host"]["min"]}),
      flush=True)
shutil.rmtree(workdir, ignore_errors=True)
