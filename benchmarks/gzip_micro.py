"""GZIP page micro-benchmark: 4096 pages (64 distinct ones, tiled) per column
shape and page size, compressed by zlib (gzip members, level 6), decoded by
gzip_decompress_into (csrc/hip/gzip.hip, a wave per page): one untimed
launch, then REPS timed ones (device events); the fastest, the median and
the slowest are reported with the output rate of the fastest. For
comparison, on the same pages: zstd_decompress_into (csrc/hip/zstd.hip) on
their zstd level-1 form, and the host decoder (inflate_ref, one thread, 64
pages, bytes objects in and out). Prints one JSON line per case."""
import json, os, sys, time, zlib

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


def gzip_page(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


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
    return min(ms), float(np.median(ms)), max(ms)


def launch_set(blocks, page):
    offs = np.concatenate(([0], np.cumsum([len(b) for b in blocks])))
    src = torch.from_numpy(np.frombuffer(b"".join(blocks), dtype=np.uint8).copy()).cuda()
    jobs = torch.tensor(
        [[offs[i % DISTINCT], len(blocks[i % DISTINCT]), i * page, page]
         for i in range(NPAGES)], dtype=torch.int64, device="cuda")
    return src, jobs, int(offs[-1])


for page in (32768, 131072):
    for name, gen in gens.items():
        pages = [gen(page) for _ in range(DISTINCT)]
        dst = torch.zeros(page * NPAGES, dtype=torch.uint8, device="cuda")

        def check():
            got = dst.view(NPAGES, page)[-DISTINCT:].cpu().numpy()
            assert all(got[i].tobytes() == pages[i] for i in range(DISTINCT))
            dst.zero_()

        gz = [gzip_page(p) for p in pages]
        src, jobs, gz_bytes = launch_set(gz, page)
        g_min, g_med, g_max = timed(lambda: hip().gzip_decompress_into(src, jobs, dst))
        check()
        zs = [cpp().zstd_compress_ref(p, 1) for p in pages]
        zsrc, zjobs, zs_bytes = launch_set(zs, page)
        z_min, z_med, z_max = timed(lambda: hip().zstd_decompress_into(zsrc, zjobs, dst))
        check()
        t0 = time.perf_counter()
        for b in gz:
            cpp().inflate_ref(b, page)
        host_s = time.perf_counter() - t0
        out = page * NPAGES
        print(json.dumps({
            "kind": name, "page": page,
            "gzip_ratio": round(page * DISTINCT / gz_bytes, 2),
            "zstd_ratio": round(page * DISTINCT / zs_bytes, 2),
            "gzip_gpu_ms": [round(g_min, 3), round(g_med, 3), round(g_max, 3)],
            "gzip_gpu_gbps": round(out / g_min / 1e6, 1),
            "zstd_gpu_ms": [round(z_min, 3), round(z_med, 3), round(z_max, 3)],
            "zstd_gpu_gbps": round(out / z_min / 1e6, 1),
            "host_1thread_gbps": round(page * DISTINCT / host_s / 1e9, 3)}), flush=True)
