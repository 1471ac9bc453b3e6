"""LZ4 blocks for the decoder tests (test_lz4.py, test_gpu_lz4.py).

entries() yields (name, block, original):

- hand-built blocks, put together sequence by sequence with `block()`;
  the expected output comes from the plain decoder `decode()` below, which
  shares no code with the project. Every one is a conforming block (it ends
  in at least 12 literals, so its last match starts at least 12 bytes and
  ends at least 5 bytes before the end) and liblz4 accepts it too;
- real blocks from pa.Codec("lz4_raw") on prefixes of the five headline
  column shapes, 200 B to 128 KB.
"""

import functools

import numpy as np
import pyarrow as pa

RNG_SEED = 4


def _len_ext(rest: int) -> bytes:
    out = b""
    while rest >= 255:
        out += b"\xff"
        rest -= 255
    return out + bytes([rest])


def seq(lits: bytes, offset: int = 0, match_len: int = 0) -> bytes:
    """One sequence; match_len == 0 makes it the block's last."""
    ll = len(lits)
    mn = match_len - 4 if match_len else 0
    assert match_len == 0 or (match_len >= 4 and 1 <= offset <= 65535)
    out = bytes([(min(ll, 15) << 4) | min(mn, 15)])
    if ll >= 15:
        out += _len_ext(ll - 15)
    out += lits
    if match_len:
        out += bytes([offset & 255, offset >> 8])
        if mn >= 15:
            out += _len_ext(mn - 15)
    return out


def decode(block: bytes) -> bytes:
    """Plain LZ4 block decoder after the format description."""
    out = bytearray()
    p, n = 0, len(block)
    while True:
        token = block[p]
        p += 1
        ll = token >> 4
        if ll == 15:
            while True:
                b = block[p]
                p += 1
                ll += b
                if b != 255:
                    break
        out += block[p:p + ll]
        p += ll
        if p == n:
            return bytes(out)
        off = block[p] | (block[p + 1] << 8)
        p += 2
        ml = token & 15
        if ml == 15:
            while True:
                b = block[p]
                p += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        assert 0 < off <= len(out)
        for _ in range(ml):
            out.append(out[-off])


TAIL = 12  # closing literals of every hand-built block


def _hand_built():
    rng = np.random.default_rng(RNG_SEED)

    def rnd(n):
        return bytes(rng.integers(0, 256, n, dtype=np.uint8))

    out = []

    def add(name, *seqs):
        blk = b"".join(seqs) + seq(rnd(TAIL))
        out.append((name, blk, decode(blk)))

    # literal lengths around the nibble and the first extension byte:
    # extension bytes 00 (15), fe (269), ff 00 (270), ff 01 (271)
    for ll in (0, 14, 15, 16, 269, 270, 271):
        add(f"lit_{ll}", seq(rnd(16), 8, 4), seq(rnd(ll), 5, 6))
    # match lengths likewise, overlapping (offset 3) and not (offset 400)
    for ml in (4, 18, 19, 20, 273, 274, 275):
        add(f"match_{ml}_ov", seq(rnd(16), 3, ml))
        add(f"match_{ml}_far", seq(rnd(400), 400, ml))
    # offsets around the copy widths and the wave size; a long and a short
    # match each. The source of each match is the literals of its own
    # sequence.
    for off in (1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65):
        add(f"off_{off}", seq(rnd(off + 3), off, 100), seq(rnd(2), off, 5))
    add("off_65535", seq(rnd(70000), 65535, 40), seq(rnd(7), 65535, 4))
    # a match whose source is the literals of the same sequence, ending at
    # the literals' last byte
    add("match_own_literals", seq(rnd(24), 24, 24))
    # a match far longer than its offset
    add("match_long_period", seq(rnd(5), 3, 5000))
    # every alignment mod 8 of the second sequence's literal run in the
    # source and the destination, and of its match
    for a in range(8):
        for b in range(8):
            add(f"align_{a}_{b}", seq(rnd(8 + a), 8 + a, 4 + b),
                seq(rnd(40), 17, 30))
    # matches only, back to back (no literals between them)
    add("matches_back_to_back", seq(rnd(20), 20, 9), seq(b"", 11, 13),
        seq(b"", 1, 4), seq(b"", 30, 70))
    out.append(("empty", b"\x00", b""))
    big = rnd(128 << 10)
    out.append(("one_literal_run_128k", seq(big), big))
    return out


def column_shapes():
    """The five headline column shapes as 128 KB of bytes each."""
    rng = np.random.default_rng(RNG_SEED + 1)
    n8, n4 = (128 << 10) // 8, (128 << 10) // 4
    return {
        "ids": np.arange(1_000_000, 1_000_000 + n8, dtype=np.int64).tobytes(),
        "f64": rng.normal(size=n8).tobytes(),
        "i32small": rng.integers(0, 100, n4, dtype=np.int32).tobytes(),
        "f32": rng.normal(size=n4).astype(np.float32).tobytes(),
        "i64wide": rng.integers(0, 10**12, n8, dtype=np.int64).tobytes(),
    }


REAL_SIZES = (200, 1000, 4096, 32768, 131072)


def _real():
    codec = pa.Codec("lz4_raw")
    out = []
    for name, data in column_shapes().items():
        for n in REAL_SIZES:
            orig = data[:n]
            out.append((f"{name}_{n}", codec.compress(orig).to_pybytes(), orig))
    return out


@functools.lru_cache(maxsize=None)
def entries():
    return tuple(_hand_built() + _real())


def liblz4_decode(block: bytes, n: int):
    """pyarrow's liblz4 on a block: the bytes, or None if it refuses."""
    try:
        return pa.Codec("lz4_raw").decompress(
            block, decompressed_size=n).to_pybytes()
    except Exception:
        return None
