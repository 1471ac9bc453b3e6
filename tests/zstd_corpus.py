"""One seeded zstd corpus shared by the CPU decoder tests
(test_zstd_dec.py) and the GPU kernel test (test_gpu.py): libzstd-compressed
payloads at three levels plus hand-assembled frames for the features the
encoder does not emit. ``zstd_frame_census`` says what each entry exercises."""

import functools

import numpy as np

from lakesoul_amd.ops import cpp

LEVELS = (1, 3, 9)

# RLE literals with the 1-, 2- and 3-byte literals header: one compressed
# block each, zero sequences (libzstd's encoder prefers an RLE *block* for
# such content, so these are assembled by hand and were checked against
# libzstd's decoder). Two frames per header length.
HAND_FRAMES = (
    ("28b52ffd20141d0000a15a00", b"Z" * 20),
    ("28b52ffda02c010000250000c5125a00", b"Z" * 300),
    ("28b52ffda0881300002d00008d38015a00", b"Z" * 5000),
    ("28b52ffd20091d0000495100", b"Q" * 9),
    ("28b52ffda0e8030000250000853e5100", b"Q" * 1000),
    ("28b52ffda0701101002d00000d17115100", b"Q" * 70000),
)


@functools.lru_cache(maxsize=None)
def payloads():
    """The payloads of test_gpu_zstd_kernel_matches_reference (seed 7), then
    small-range int32 pages (many short matches and repeat offsets: FSE,
    RLE and repeat sequence tables, treeless literals)."""
    rng = np.random.default_rng(7)
    out = []
    out.append(rng.integers(0, 256, 100000, dtype=np.uint8).tobytes())
    out.append(b"\x42" * 200000)
    out.append(np.arange(50000, dtype=np.int64).tobytes())
    out.append(rng.normal(size=40000).tobytes())
    out.append(bytes(rng.integers(65, 70, 150000, dtype=np.uint8)))
    words = [b"lake", b"soul", b"gpu", b"zstd", b"merge"]
    out.append(b" ".join(words[i] for i in rng.integers(0, 5, 80000)))
    out.append(b"x" * 300000)  # multi-block RLE
    for n in rng.integers(1, 5000, 40):
        out.append(bytes(rng.integers(0, 8, int(n), dtype=np.uint8)))
    rng = np.random.default_rng(11)
    out.append(rng.integers(0, 500, 65536).astype(np.int32).tobytes())
    # second producer of a repeat-mode offset table (level 9)
    rng = np.random.default_rng(13)
    out.append(b" ".join(words[i] for i in rng.integers(0, 5, 80000)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def corpus():
    """Tuple of (name, compressed frame, original bytes)."""
    entries = [(f"hand{i}", bytes.fromhex(h), orig)
               for i, (h, orig) in enumerate(HAND_FRAMES)]
    for level in LEVELS:
        for i, p in enumerate(payloads()):
            entries.append((f"p{i}_l{level}", cpp().zstd_compress_ref(p, level), p))
    return tuple(entries)
