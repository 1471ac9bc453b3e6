"""Huffman-only zstd page micro-benchmark: 4096 pages (64 distinct ones,
tiled) per payload kind and page size, level-1 frames, decoded by one timed
launch each of zstd_huf_decompress_into (a workgroup per page, 64 lanes per
Huffman stream) and of zstd_decompress_into (a wave per page, one lane per
stream), after one untimed launch of each. Prints one JSON line per case."""
import json, os, sys

import numpy as np, torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lakesoul_amd.ops import cpp, hip

rng = np.random.default_rng(0)
NPAGES, DISTINCT = 4096, 64
gens = {
    "v_f64_normal": lambda n: rng.normal(size=n // 8).tobytes(),
    "f_f32_normal": lambda n: rng.normal(size=n // 4).astype(np.float32).tobytes(),
    "t_i64_lt1e12": lambda n: rng.integers(0, 10**12, n // 8).astype(np.int64).tobytes(),
}


def timed(fn):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    st = fn()
    b.record()
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0
    return a.elapsed_time(b)


for page in (32768, 131072):
    for name, gen in gens.items():
        # the encoder finds a match in some int64 pages: those carry
        # sequences and are not this kernel's pages ("huf_only" below)
        pages, frames, tried = [], [], 0
        while len(pages) < DISTINCT and tried < 8 * DISTINCT:
            p = gen(page)
            f = cpp().zstd_compress_ref(p, 1)
            tried += 1
            if cpp().zstd_huf_only(f, page):
                pages.append(p)
                frames.append(f)
        assert len(pages) == DISTINCT, name
        offs = np.concatenate(([0], np.cumsum([len(f) for f in frames])))
        src = torch.from_numpy(np.frombuffer(b"".join(frames), dtype=np.uint8).copy()).cuda()
        jobs = torch.tensor(
            [[offs[i % DISTINCT], len(frames[i % DISTINCT]), i * page, page]
             for i in range(NPAGES)], dtype=torch.int64, device="cuda")
        dst = torch.zeros(page * NPAGES, dtype=torch.uint8, device="cuda")
        ms_new = timed(lambda: hip().zstd_huf_decompress_into(src, jobs, dst))
        got = dst.view(NPAGES, page)[:DISTINCT].cpu().numpy()
        assert all(got[i].tobytes() == pages[i] for i in range(DISTINCT))
        ms_old = timed(lambda: hip().zstd_decompress_into(src, jobs, dst))
        out = page * NPAGES
        print(json.dumps({
            "kind": name, "page": page, "huf_only": round(DISTINCT / tried, 2),
            "ratio": round(page * DISTINCT / int(offs[-1]), 2),
            "huf_ms": round(ms_new, 3), "huf_gbps": round(out / ms_new / 1e6, 1),
            "old_ms": round(ms_old, 3), "old_gbps": round(out / ms_old / 1e6, 1),
            "speedup": round(ms_old / ms_new, 1)}), flush=True)
