"""LZ4_RAW page micro-benchmark: 4096 pages (64 distinct ones, tiled) per
column shape and page size, compressed by the project's encoder, decoded by
lz4_decompress_into (csrc/hip/lz4.hip, a wave per page): one untimed launch,
then REPS timed ones (device events); the fastest and the median are
reported with the output rate of the fastest. For comparison the host
decoder (lz4_block_decode_ref, one thread, 64 pages, bytes objects in and
out). Prints one JSON line per case."""
import json, os, sys, time

import numpy as np, torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lakesoul_amd.ops import cpp, hip

rng = np.random.default_rng(0)
NPAGES, DISTINCT, REPS = 4096, 64, 7
_next_id = [0]


def _ids(n):
    a = np.arange(_next_id[0], _next_id[0] + n // 8, dtype=np.int64)
    _next_id[0] += n // 8
    return a.tobytes()


gens = {
    "id_i64_sorted": _ids,
    "v_f64_normal": lambda n: rng.normal(size=n // 8).tobytes(),
    "k_i32_lt1000": lambda n: rng.integers(0, 1000, n // 4, dtype=np.int32).tobytes(),
    "f_f32_normal": lambda n: rng.normal(size=n // 4).astype(np.float32).tobytes(),
    "t_i64_lt1e12": lambda n: rng.integers(0, 10**12, n // 8).astype(np.int64).tobytes(),
}


def timed(fn):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        st = fn()
        b.record()
        torch.cuda.synchronize()
        assert int((st != 0).sum()) == 0
        ms.append(a.elapsed_time(b))
    return min(ms), float(np.median(ms))


for page in (32768, 131072):
    for name, gen in gens.items():
        pages = [gen(page) for _ in range(DISTINCT)]
        blocks = [cpp().lz4_compress_ref(p) for p in pages]
        offs = np.concatenate(([0], np.cumsum([len(b) for b in blocks])))
        src = torch.from_numpy(np.frombuffer(b"".join(blocks), dtype=np.uint8).copy()).cuda()
        jobs = torch.tensor(
            [[offs[i % DISTINCT], len(blocks[i % DISTINCT]), i * page, page]
             for i in range(NPAGES)], dtype=torch.int64, device="cuda")
        dst = torch.zeros(page * NPAGES, dtype=torch.uint8, device="cuda")
        ms_min, ms_med = timed(lambda: hip().lz4_decompress_into(src, jobs, dst))
        got = dst.view(NPAGES, page)[-DISTINCT:].cpu().numpy()
        assert all(got[i].tobytes() == pages[i] for i in range(DISTINCT))
        t0 = time.perf_counter()
        for b in blocks:
            cpp().lz4_block_decode_ref(b, page)
        host_s = time.perf_counter() - t0
        out = page * NPAGES
        print(json.dumps({
            "kind": name, "page": page,
            "ratio": round(page * DISTINCT / int(offs[-1]), 2),
            "gpu_ms_min": round(ms_min, 3), "gpu_ms_median": round(ms_med, 3),
            "gpu_gbps": round(out / ms_min / 1e6, 1),
            "host_1thread_gbps": round(page * DISTINCT / host_s / 1e9, 2)}), flush=True)
