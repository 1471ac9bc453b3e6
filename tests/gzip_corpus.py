"""GZIP pages for the decoder tests (test_gzip.py, test_gpu_gzip.py).

entries() yields (name, page, original):

- pages from zlib.compressobj: levels 0, 1, 6 and 9, the strategies Z_FIXED,
  Z_HUFFMAN_ONLY and Z_RLE, gzip (wbits 31) and zlib (wbits 15) framing, a
  Z_SYNC_FLUSH and a Z_FULL_FLUSH in the middle, two members back to back, a
  member whose header carries FEXTRA, FNAME, FCOMMENT and FHCRC;
- hand-assembled DEFLATE streams, put together bit by bit with BitWriter
  and wrapped into a gzip member: what zlib's encoder never emits (a 15-bit
  code, a distance of 32768, a repeat code that runs from the literal/length
  lengths into the distance lengths). Their expected output comes from
  zlib's decoder, which shares no code with the project.
"""

import functools
import struct
import zlib

import numpy as np

from lz4_corpus import column_shapes

RNG_SEED = 12


# ---- framing ---------------------------------------------------------- #

def gzip_member(raw: bytes, orig: bytes, *, extra=None, name=None,
                comment=None, hcrc=False) -> bytes:
    """A gzip member around the bare DEFLATE stream `raw` of `orig`."""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | \
          (16 if comment is not None else 0) | (2 if hcrc else 0)
    head = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 3])
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if name is not None:
        head += name + b"\0"
    if comment is not None:
        head += comment + b"\0"
    if hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + raw + struct.pack("<II", zlib.crc32(orig), len(orig) & 0xFFFFFFFF)


def deflate(data: bytes, level=6, wbits=31, strategy=zlib.Z_DEFAULT_STRATEGY,
            flush_at=None, flush_mode=zlib.Z_SYNC_FLUSH) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return (c.compress(data[:flush_at]) + c.flush(flush_mode) +
            c.compress(data[flush_at:]) + c.flush())


def zlib_decode(page: bytes):
    """zlib's bytes for a page (gzip members or one zlib stream, nothing
    behind them), or None if it refuses."""
    try:
        out = b""
        rest = page
        first = True
        while rest:
            if not first and rest[:2] != b"\x1f\x8b":
                return None
            d = zlib.decompressobj(47)  # gzip or zlib by the header
            out += d.decompress(rest)
            if not d.eof:
                return None
            if page[:2] != b"\x1f\x8b" and d.unused_data:
                return None
            rest = d.unused_data
            first = False
        return out if not first else None
    except zlib.error:
        return None


# ---- hand-assembled DEFLATE ------------------------------------------- #

class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, count):
        """`count` bits of value, least significant first (header fields,
        extra bits)."""
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """A Huffman code: most significant bit first."""
        rev = int(format(code, f"0{length}b")[::-1], 2)
        self.bits(rev, length)

    def to_bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lens):
    """{symbol: (code, length)} of the canonical code with these lengths."""
    out, code = {}, 0
    for length in range(1, 16):
        for sym, l in enumerate(lens):
            if l == length:
                out[sym] = (code, length)
                code += 1
        code <<= 1
    return out


def _complete_lengths(symbols):
    """Lengths of a complete code over `symbols` (at least two)."""
    m = len(symbols)
    k = m.bit_length() - 1
    r = m - (1 << k)
    return {s: (k + 1 if i < 2 * r else k) for i, s in enumerate(symbols)}


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51,
            59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385,
             513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385,
             24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def put_symbols(w, lit, dist, symbols):
    """symbols: ints (literals), (length, distance) pairs; 256 is added."""
    for s in symbols:
        if isinstance(s, int):
            w.code(*lit[s])
            continue
        length, distance = s
        li = max(i for i, b in enumerate(LEN_BASE) if b <= length)
        if length == 258:
            li = 28
        w.code(*lit[257 + li])
        w.bits(length - LEN_BASE[li], LEN_EXTRA[li])
        di = max(i for i, b in enumerate(DIST_BASE) if b <= distance)
        w.code(*dist[di])
        w.bits(distance - DIST_BASE[di], DIST_EXTRA[di])
    w.code(*lit[256])


def dynamic_block(w, cl_tokens, hlit, hdist, lit_lens, dist_lens, symbols,
                  last=True):
    """One dynamic block. cl_tokens spell lit_lens + dist_lens in the
    code-length alphabet: (symbol, extra value) pairs."""
    w.bits(1 if last else 0, 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(19 - 4, 4)
    used = sorted({s for s, _ in cl_tokens})
    if len(used) == 1:
        used.append((used[0] + 1) % 19)
    cl_len = _complete_lengths(used)
    for s in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
        w.bits(cl_len.get(s, 0), 3)
    cl = canonical([cl_len.get(s, 0) for s in range(19)])
    for s, extra in cl_tokens:
        w.code(*cl[s])
        if s >= 16:
            w.bits(extra, {16: 2, 17: 3, 18: 7}[s])
    put_symbols(w, canonical(lit_lens), canonical(dist_lens), symbols)


def fixed_block(w, symbols, last=True):
    w.bits(1 if last else 0, 1)
    w.bits(1, 2)
    lit = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
    put_symbols(w, lit, canonical([5] * 32), symbols)


def raw_15bit_code():
    """Literal/length lengths 1, 2, ..., 14, 15, 15: the two longest codes
    have 15 bits (symbol 14 and the end of block). No distance code."""
    lit_lens = list(range(1, 16)) + [0] * 241 + [15]
    tokens = [(l, 0) for l in range(1, 16)] + [(18, 138 - 11), (18, 103 - 11), (15, 0)]
    tokens.append((0, 0))  # HDIST = 1: one distance length, zero
    w = BitWriter()
    rng = np.random.default_rng(RNG_SEED)
    msg = [int(x) for x in rng.integers(0, 15, 300)] + [14, 14, 13, 14, 0]
    dynamic_block(w, tokens, 257, 1, lit_lens, [0], msg)
    return w.to_bytes()


def raw_single_distance_code():
    """One distance code of one bit (zlib's encoder emits this for a block
    whose matches all use one distance code)."""
    lit_lens = [0] * 97 + [1] + [0] * 158 + [2, 2]
    tokens = [(18, 97 - 11), (1, 0), (18, 138 - 11), (18, 20 - 11), (2, 0), (2, 0),
              (1, 0)]
    w = BitWriter()
    dynamic_block(w, tokens, 258, 1, lit_lens, [1], [97, (3, 1), 97, (3, 1)])
    return w.to_bytes()


def raw_repeat_across_hlit():
    """The repeat code 16 behind lens[256] = 3 covers lens[257] and the
    first two distance lengths."""
    lit_lens = [0] * 97 + [1, 2] + [0] * 157 + [3, 3]
    dist_lens = [3, 3, 2, 1]
    tokens = [(18, 97 - 11), (1, 0), (2, 0), (18, 138 - 11), (18, 19 - 11),
              (3, 0), (16, 0), (2, 0), (1, 0)]
    w = BitWriter()
    msg = [97, 98, 97, 98, (3, 4), (3, 1), 98, (3, 2), (3, 3)]
    dynamic_block(w, tokens, 258, 4, lit_lens, dist_lens, msg)
    return w.to_bytes()


def raw_far_long_matches():
    """About 100 KB: 32768 random literals, then matches of length 258 at
    distance 32768 (zlib's encoder stops at 32506), fixed Huffman codes."""
    rng = np.random.default_rng(RNG_SEED + 1)
    head = [int(x) for x in rng.integers(0, 256, 32768, dtype=np.uint8)]
    w = BitWriter()
    fixed_block(w, head, last=False)
    fixed_block(w, [(258, 32768)] * 130 + [7, (258, 1), (258, 32768)] +
                [(258, 32768)] * 129 + [(3, 32768), (4, 32767)])
    return w.to_bytes()


def _hand_assembled():
    out = []
    for name, raw in (("hand_15bit_code", raw_15bit_code()),
                      ("hand_single_distance_code", raw_single_distance_code()),
                      ("hand_repeat_across_hlit", raw_repeat_across_hlit()),
                      ("hand_far_long_matches", raw_far_long_matches())):
        orig = zlib.decompressobj(-15).decompress(raw)
        out.append((name, gzip_member(raw, orig), orig))
    return out


# ---- zlib-made pages -------------------------------------------------- #

def _zlib_made():
    rng = np.random.default_rng(RNG_SEED + 2)
    shapes = column_shapes()
    out = []

    def add(name, page, orig):
        out.append((name, page, orig))

    for sname, data in shapes.items():
        for n in (200, 4096, 131072):
            add(f"{sname}_{n}", deflate(data[:n]), data[:n])
        part = data[:32768]
        for level in (0, 1, 9):
            add(f"{sname}_level{level}", deflate(part, level), part)
        add(f"{sname}_fixed", deflate(part, strategy=zlib.Z_FIXED), part)
        add(f"{sname}_huffman_only", deflate(part, strategy=zlib.Z_HUFFMAN_ONLY), part)
        add(f"{sname}_rle", deflate(part, strategy=zlib.Z_RLE), part)
        add(f"{sname}_zlib", deflate(part, wbits=15), part)
        add(f"{sname}_sync_flush", deflate(part, flush_at=10_001), part)
        add(f"{sname}_full_flush",
            deflate(part, flush_at=777, flush_mode=zlib.Z_FULL_FLUSH), part)
    ids, small = shapes["ids"], shapes["i32small"]
    add("two_members", deflate(ids[:5000]) + deflate(small[:3001], 1),
        ids[:5000] + small[:3001])
    add("three_members_one_empty", deflate(ids[:100]) + deflate(b"") + deflate(small[:64]),
        ids[:100] + small[:64])
    part = small[:9000]
    add("header_fields",
        gzip_member(deflate(part, wbits=-15), part, extra=b"ab\x04\x00wxyz",
                    name=b"page.bin", comment=b"a comment", hcrc=True), part)
    add("header_name_only",
        gzip_member(deflate(part, wbits=-15), part, name=b""), part)
    add("empty", deflate(b""), b"")
    add("empty_zlib", deflate(b"", wbits=15), b"")
    add("one_byte", deflate(b"\x07"), b"\x07")
    lit = bytes(rng.permutation(256).astype(np.uint8))
    add("literals_64", deflate(lit[:64], strategy=zlib.Z_HUFFMAN_ONLY), lit[:64])
    add("literals_65", deflate(lit[:65], strategy=zlib.Z_HUFFMAN_ONLY), lit[:65])
    add("literals_64_fixed", deflate(lit[:64], strategy=zlib.Z_FIXED), lit[:64])
    noise = bytes(rng.integers(0, 256, 200_000, dtype=np.uint8))
    add("random_200k", deflate(noise), noise)          # stored blocks
    add("random_200k_level0", deflate(noise, 0), noise)
    add("equal_100k", deflate(b"\xab" * 100_000, 9), b"\xab" * 100_000)
    per = bytes(range(13)) * 4000
    add("period13", deflate(per), per)
    return out


@functools.lru_cache(maxsize=None)
def entries():
    return tuple(_hand_assembled() + _zlib_made())
