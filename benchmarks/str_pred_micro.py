"""String predicates: the kernel (csrc/hip/str_pred.hip) timed with device
events, the mean-length threshold between its two shapes, and Cmp.evaluate /
a filtered scan against the Python loop the string branch of Cmp.evaluate
used to be (kept here as `loop_evaluate`). One JSON line per measurement.

    python benchmarks/str_pred_micro.py [--part kernel,sweep,evaluate,cpu,scan]
                                        [--rows 8000000] [--reps 9]

kernel   : 8 M rows of 7 short values, 8 M keys of ~40 bytes, rows/8 values of
           ~1 KB; eq, IN of 16, IN of 1000, 'abc%', '%abc%'; both shapes;
           GB/s of offsets + bytes (what a predicate that reads every byte
           has to read; eq on a length mismatch reads less)
sweep    : ~256 MB columns of one fixed value length each; a compare that
           runs to the last byte and a '%abc%' that finds nothing
evaluate : Cmp.evaluate on a CUDA batch, rows/8 rows, new against the loop
cpu      : the host twin against the loop, rows/8 rows
scan     : a filtered scan of a `rows`-row string table, end to end
"""
import argparse, json, os, sys, tempfile, time

import numpy as np, torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lakesoul_amd.io.batch import Batch, Column
from lakesoul_amd.io.filters import Cmp, Like
from lakesoul_amd.io.schema import Field, Schema
from lakesoul_amd.ops import cpp

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="kernel,sweep,evaluate,cpu,scan")
ap.add_argument("--rows", type=int, default=8_000_000)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--rehearse", action="store_true",
                help="no GPU: run the host parts only (checks the script, times nothing)")
args = ap.parse_args()
parts = set(args.part.split(","))
if args.rehearse:
    parts &= {"cpu"}
else:
    assert torch.cuda.is_available(), "str_pred_micro.py measures on the GPU"
    from lakesoul_amd.ops import hip
    dev = torch.device("cuda:0")
rng = np.random.default_rng(0)
n = args.rows
OPS = {"eq": 0, "lt": 2, "in": 6, "like": 7}
MODES = ["AIR", "R", "TRUCK", "MAIL", "SHIP", "REG AIR", "FOB-EXPORT"]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def dict7(rows):
    words = [np.frombuffer(m.encode(), dtype=np.uint8) for m in MODES]
    pick = rng.integers(0, 7, rows)
    lens = np.array([len(w) for w in words])[pick]
    offs = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    blob = np.zeros(int(offs[-1]), dtype=np.uint8)
    for k, w in enumerate(words):
        starts = offs[:-1][pick == k]
        for j, b in enumerate(w):
            blob[starts + j] = b
    return offs.astype(np.int32), blob


def keys40(rows):
    width = 44
    m = np.empty((rows, width), dtype=np.uint8)
    prefix = np.frombuffer(b"tenant-0001/region-eu-west/key-", dtype=np.uint8)
    m[:, :len(prefix)] = prefix
    i = np.arange(rows, dtype=np.int64)
    for d in range(width - len(prefix)):
        m[:, width - 1 - d] = 48 + (i // 10 ** d) % 10
    lens = 36 + (i * 5) % 9
    offs = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return offs.astype(np.int32), m[np.arange(width)[None, :] < lens[:, None]]


def values1k(rows):
    lens = 1000 + (np.arange(rows, dtype=np.int64) * 11) % 49
    offs = np.zeros(rows + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    return offs.astype(np.int32), rng.integers(97, 123, int(offs[-1]), dtype=np.uint8)


def row_of(offs, blob, i):
    return blob[offs[i]:offs[i + 1]].tobytes()


def operands(offs, blob):
    """eq / IN literals are rows of the column itself, so they do match."""
    rows = len(offs) - 1
    at = lambda k: row_of(offs, blob, (k * 7919) % rows)
    return {
        "eq": (OPS["eq"], cpp().str_pred_compile_literal(at(1))),
        "in16": (OPS["in"], cpp().str_pred_compile_set([at(k) for k in range(16)])),
        "in1000": (OPS["in"], cpp().str_pred_compile_set(
            [at(k) for k in range(500)] + [b"no-such-value-%d" % k for k in range(500)])),
        "like abc%": (OPS["like"], cpp().str_pred_compile_like(b"abc%", 92, True)),
        "like %abc%": (OPS["like"], cpp().str_pred_compile_like(b"%abc%", 92, True)),
    }


def time_kernel(o, b, op, operand, shape, reps):
    ob, om = (t.to(dev) for t in operand)
    out = torch.empty(o.numel() - 1, dtype=torch.bool, device=dev)
    for _ in range(2):
        hip().str_pred_mask(o, b, None, op, ob, om, shape=shape, out=out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        hip().str_pred_mask(o, b, None, op, ob, om, shape=shape, out=out)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms)), out


if "kernel" in parts:
    for name, make, rows in (("dict7", dict7, n), ("key40", keys40, n),
                             ("value1k", values1k, max(n // 8, 1))):
        offs, blob = make(rows)
        o, b = torch.from_numpy(offs).to(dev), torch.from_numpy(blob).to(dev)
        read = offs.nbytes + blob.nbytes
        for opname, (op, operand) in operands(offs, blob).items():
            ref = None
            for shape in ("rows", "wave"):
                med, lo, hi, out = time_kernel(o, b, op, operand, shape, args.reps)
                if ref is None:
                    ref = out.clone()
                assert torch.equal(ref, out), (name, opname)     # the shapes agree
                emit(part="kernel", data=name, rows=rows, op=opname, shape=shape,
                     mean_len=round(blob.nbytes / rows, 1), median_ms=round(med, 3),
                     min_ms=round(lo, 3), max_ms=round(hi, 3),
                     read_mb=round(read / 1e6, 1), gb_per_s=round(read / med / 1e6, 1),
                     selected=int(out.sum()))
        del o, b

if "sweep" in parts:
    total = 256 << 20
    for length in (8, 16, 32, 64, 96, 128, 192, 256, 384, 512, 1024, 4096):
        rows = total // length
        blob = rng.integers(97, 123, rows * length, dtype=np.uint8)
        lit = rng.integers(97, 123, length, dtype=np.uint8)
        m = blob.reshape(rows, length)
        m[::2, :] = lit                      # half the rows: the literal ...
        m[::2, -1] = 96                      # ... but for a smaller last byte
        offs = (np.arange(rows + 1, dtype=np.int64) * length).astype(np.int32)
        o, b = torch.from_numpy(offs).to(dev), torch.from_numpy(blob).to(dev)
        cases = {"lt (to the last byte)": (OPS["lt"], cpp().str_pred_compile_literal(lit.tobytes())),
                 "like %ABC% (no match)": (OPS["like"], cpp().str_pred_compile_like(b"%ABC%", 92, True))}
        for opname, (op, operand) in cases.items():
            t = {}
            for shape in ("rows", "wave"):
                t[shape], _, _, out = time_kernel(o, b, op, operand, shape, args.reps)
            emit(part="sweep", value_len=length, rows=rows, op=opname,
                 rows_ms=round(t["rows"], 3), wave_ms=round(t["wave"], 3),
                 faster="rows" if t["rows"] <= t["wave"] else "wave")
        del o, b


def loop_evaluate(c, op, value):
    """The string branch of Cmp.evaluate before the kernel: copy the column
    to the host, one bytes object per row, compare in a Python loop."""
    offs = c.offsets.cpu().numpy()
    bys = c.bytes_.cpu().numpy().tobytes()
    v = value.encode() if isinstance(value, str) else bytes(value)
    vals = [bys[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    f = {"eq": lambda a: a == v, "lt": lambda a: a < v}[op]
    out = torch.from_numpy(np.array([f(x) for x in vals])).to(c.bytes_.device)
    if c.validity is not None:
        out = out & c.validity.to(torch.bool)
    return out


def wall(fn, reps, sync):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts)), out


for part, device in (("evaluate", None), ("cpu", torch.device("cpu"))):
    if part not in parts:
        continue
    device = device or dev
    rows = max(n // 8, 1)
    for name, make, lit in (("dict7", dict7, "MAIL"), ("key40", keys40, None)):
        offs, blob = make(rows)
        lit = lit or row_of(offs, blob, rows // 2).decode()
        col = Column("string", offsets=torch.from_numpy(offs).to(device),
                     bytes_=torch.from_numpy(blob).to(device))
        batch = Batch(Schema([Field("s", "string")]), {"s": col})
        for op in ("eq", "lt"):
            e = Cmp("s", op, lit)
            e.evaluate(batch)                                  # warm: compile, upload
            new = wall(lambda: e.evaluate(batch), args.reps, device.type == "cuda")
            old = wall(lambda: loop_evaluate(col, op, lit), 2, device.type == "cuda")
            assert torch.equal(new[3], old[3])
            emit(part=part, data=name, rows=rows, op=op, new_median_ms=round(new[0], 3),
                 new_min_ms=round(new[1], 3), new_max_ms=round(new[2], 3),
                 loop_median_ms=round(old[0], 1), loop_over_new=round(old[0] / new[0], 1))
        e = Like("s", "%AI%" if name == "dict7" else "%key-%77")
        e.evaluate(batch)
        new = wall(lambda: e.evaluate(batch), args.reps, device.type == "cuda")
        emit(part=part, data=name, rows=rows, op="like " + e.pattern,
             new_median_ms=round(new[0], 3), selected=int(new[3].sum()))

if "scan" in parts:
    from lakesoul_amd.meta.client import MetaClient
    from lakesoul_amd.meta.store import SqliteMetaStore
    from lakesoul_amd.tables.catalog import LakeSoulCatalog

    with tempfile.TemporaryDirectory() as td:
        catalog = LakeSoulCatalog(MetaClient(SqliteMetaStore(os.path.join(td, "meta.db"))),
                                  warehouse=os.path.join(td, "wh"))
        t = catalog.create_table("strs", Schema([Field("id", "int64", False),
                                                 Field("s", "string")]),
                                 primary_keys=["id"], hash_bucket_num=4)
        import pyarrow as pa

        modes = pa.array(MODES).take(pa.array(rng.integers(0, 7, n)))
        t.upsert(pa.table({"id": pa.array(np.arange(n, dtype=np.int64)), "s": modes}),
                 device="cuda")

        def scan():
            return t.scan(filters=[("s", "=", "MAIL")], device="cuda").to_arrow().num_rows

        scan()
        new = wall(scan, 3, True)
        plain = wall(lambda: t.scan(device="cuda").to_arrow().num_rows, 3, True)
        kernel_eval = Cmp.evaluate

        def old_eval(self, batch):
            c = batch.columns[self.col]
            return loop_evaluate(c, self.op, self.value) if c.is_string else kernel_eval(self, batch)

        Cmp.evaluate = old_eval
        try:
            old = wall(scan, 1, True)
        finally:
            Cmp.evaluate = kernel_eval
        assert old[3] == new[3]
        emit(part="scan", rows=n, selected=new[3], unfiltered_scan_ms=round(plain[0], 1),
             new_median_ms=round(new[0], 1), new_min_ms=round(new[1], 1),
             new_max_ms=round(new[2], 1), loop_ms=round(old[0], 1),
             loop_over_new=round(old[0] / new[0], 1))
