"""Huffman-only zstd frames shared by tests/test_huf_par.py (host twin) and
tests/test_gpu_huf.py (kernel): level-1 frames of prefixes of seeded byte
sources, compressed by the writer's own libzstd."""

import functools

import numpy as np

from lakesoul_amd.ops import cpp

LENGTHS = (200, 256, 300, 1000, 1021, 1022, 1023, 1024, 1025, 4096, 16383,
           16384, 65536, 131072)
_N = max(LENGTHS)


def _geometric(rng, p):
    return np.minimum(rng.geometric(p, _N) - 1, 255).astype(np.uint8).tobytes()


def sources():
    """name -> 128 KB of bytes, each from its own seed."""
    out = {}
    out["f64"] = np.random.default_rng(11).normal(size=_N // 8).tobytes()
    out["f32"] = (np.random.default_rng(12).normal(size=_N // 4)
                  .astype(np.float32).tobytes())
    out["i64"] = (np.random.default_rng(13).integers(0, 10 ** 12, _N // 8)
                  .astype(np.int64).tobytes())
    out["geo08"] = _geometric(np.random.default_rng(14), 0.08)
    out["u16"] = (np.random.default_rng(15).integers(0, 16, _N)
                  .astype(np.uint8).tobytes())
    out["u40"] = (np.random.default_rng(16).integers(0, 40, _N)
                  .astype(np.uint8).tobytes())
    return out


def geometric_source(p, seed=17):
    return _geometric(np.random.default_rng(seed), p)


@functools.lru_cache(maxsize=None)
def entries():
    """[(name, frame, original)] for every source and prefix length, whether
    the classifier accepts the frame or not."""
    out = []
    for sname, data in sources().items():
        for n in LENGTHS:
            orig = data[:n]
            out.append((f"{sname}_{n}", cpp().zstd_compress_ref(orig, 1), orig))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def accepted():
    return tuple(e for e in entries() if cpp().zstd_huf_only(e[1], len(e[2])))
