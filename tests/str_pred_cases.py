"""Case tables and plain-Python models for the string predicates
(csrc/cpp/str_pred.h, csrc/hip/str_pred.hip), shared by test_str_pred.py
(host twin) and test_gpu_str_pred.py (kernel, both shapes).

Models: comparison is Python ``bytes`` comparison; LIKE is translated to
``re`` with ``re.DOTALL``, over ``str`` for string columns and over
``bytes`` for binary ones."""

import re

import numpy as np
import torch

CMP_OPS = ["eq", "noteq", "lt", "lteq", "gt", "gteq"]
OP_CODE = {"eq": 0, "noteq": 1, "lt": 2, "lteq": 3, "gt": 4, "gteq": 5, "in": 6,
           "like": 7, "notlike": 8}

VALUE_LENGTHS = [0, 1, 3, 4, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257]
LITERAL_LENGTHS = [0, 1, 4, 8, 9, 65]
ROW_COUNTS = [1, 63, 64, 65, 257]
EDGE_BYTES = [0x00, 0x7F, 0x80, 0xFF]
_CYCLE = bytes([0x61, 0x00, 0x7F, 0x80, 0xFF, 0x62, 0x63])


def literal_of(length: int) -> bytes:
    return bytes(_CYCLE[i % len(_CYCLE)] for i in range(length))


# --------------------------------------------------------------------- #
# models


def model_cmp(vals, op, lit):
    f = {"eq": lambda a: a == lit, "noteq": lambda a: a != lit,
         "lt": lambda a: a < lit, "lteq": lambda a: a <= lit,
         "gt": lambda a: a > lit, "gteq": lambda a: a >= lit}[op]
    return [v is not None and f(v) for v in vals]


def model_in(vals, lits):
    s = set(lits)
    return [v is not None and v in s for v in vals]


def like_regex(pattern, escape="\\"):
    """LIKE pattern (str or bytes) -> compiled regex of the same type."""
    binary = isinstance(pattern, bytes)
    units = [pattern[i:i + 1] for i in range(len(pattern))]
    esc = (escape.encode() if binary else escape) if escape else None
    pct, und = (b"%", b"_") if binary else ("%", "_")
    out = []
    i = 0
    while i < len(units):
        u = units[i]
        if esc is not None and u == esc:
            if i + 1 < len(units):
                i += 1
            out.append(re.escape(units[i]))
        elif u == pct:
            out.append(b".*" if binary else ".*")
        elif u == und:
            out.append(b"." if binary else ".")
        else:
            out.append(re.escape(u))
        i += 1
    return re.compile((b"" if binary else "").join(out), re.DOTALL)


def model_like(vals, pattern, negate=False, escape="\\", binary=False):
    """vals are bytes (None = NULL); pattern str or bytes."""
    pat = pattern.encode() if isinstance(pattern, str) else pattern
    if binary:
        rx = like_regex(pat, escape)
        hit = [v is not None and rx.fullmatch(v) is not None for v in vals]
    else:
        rx = like_regex(pat.decode("utf-8"), escape)
        hit = [v is not None and rx.fullmatch(v.decode("utf-8")) is not None
               for v in vals]
    return [v is not None and (h != negate) for v, h in zip(vals, hit)]


# --------------------------------------------------------------------- #
# columns


def phased(values):
    """Every value at every byte phase 0..7 of its 8-byte word: in front of
    each copy goes a filler value of the length that puts it there. Returns
    the row list (fillers included)."""
    rows, at = [], 0
    for v in values:
        for ph in range(8):
            pad = (ph - at) % 8
            rows.append(bytes([0x70 + ph]) * pad)
            at += pad
            assert at % 8 == ph
            rows.append(v)
            at += len(v)
    return rows


def column(rows, offs_dtype=torch.int32, base_rows=0, null_every=0):
    """rows (bytes, None = NULL) -> (offsets, bytes, validity-or-None, rows
    as the model sees them). base_rows > 0 puts that many junk rows in front
    and returns the offsets of a slice behind them, so offsets[0] != 0.
    null_every = k marks every k-th row NULL too (it keeps its bytes)."""
    junk = [b"junk-%d" % i for i in range(base_rows)]
    seen = [None if (r is None or (null_every and i % null_every == 0)) else r
            for i, r in enumerate(rows)]
    raw = junk + [r if r is not None else b"" for r in rows]
    offs = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in raw], out=offs[1:])
    blob = b"".join(raw)
    by = (torch.frombuffer(bytearray(blob), dtype=torch.uint8) if blob
          else torch.empty(0, dtype=torch.uint8))
    offsets = torch.from_numpy(offs).to(offs_dtype)[base_rows:].clone()
    validity = None
    if any(s is None for s in seen):
        validity = torch.tensor([0 if s is None else 1 for s in seen],
                                dtype=torch.uint8)
    return offsets, by, validity, seen


# --------------------------------------------------------------------- #
# comparison cases


def cmp_values(lit: bytes):
    """Values around one literal: equal, proper prefix either way, first /
    last byte different with the edge bytes, and every listed length built
    from the literal's own bytes (so the compare runs deep) with and without
    a changed last byte."""
    vals = [lit, lit + b"\x00", lit + b"\xff", b"", b"\x00", b"\xff"]
    if lit:
        vals += [lit[:-1], lit[:len(lit) // 2]]
        for e in EDGE_BYTES:
            vals.append(bytes([e]) + lit[1:])
            vals.append(lit[:-1] + bytes([e]))
    rep = (lit or b"\x61") * (257 // max(len(lit), 1) + 2)
    for n in VALUE_LENGTHS:
        v = rep[:n]
        vals.append(v)
        if n:
            vals.append(v[:-1] + bytes([v[-1] ^ 0x80]))
    return vals


def in_sets():
    big = [b"key-%036d" % (i * 7919 % 100003) for i in range(1000)]  # 40 bytes each
    return {
        "empty": [],
        "one": [b"abc"],
        "two": [b"b", b"a\xff"],
        "seven": [b"", b"a", b"ab", b"abc", b"\x80", b"\xff\xff", b"zz" * 40],
        "dups": [b"x", b"abc", b"x", b"abc", b"x"],
        "empty_member": [b""],
        "big": big,
    }


def in_values(lits):
    vals = [b"", b"a", b"ab", b"abc", b"abd", b"x", b"\x80", b"\xff", b"\xff\xff",
            b"zz" * 40, b"zz" * 39, b"a\xff", b"b", b"c"]
    for l in lits[:5] + lits[-5:] + lits[len(lits) // 2:len(lits) // 2 + 3]:
        vals += [l, l + b"0", l[:-1]]
    return vals


# --------------------------------------------------------------------- #
# LIKE cases

LIKE_PATTERNS = [
    "", "%", "_", "a", "a%", "%a", "%a%", "a%b", "a_c", "%_%", "__",
    "%ab%ab%", "a%a", "%%", "_%", "%_", "a%b%c", "%ab", "ab%", "_b_", "%a_c%",
    "\\%", "\\_", "\\\\", "a\\%", "%\\_%", "a\\\\b", "\\a", "ab\\", "%\\%%",
    "a_", "_c", "%é%", "é_", "_€_", "%😀", "___",
]
LIKE_STRINGS = [
    "", "a", "b", "ab", "ba", "abc", "aXc", "a_c", "a%", "%", "_", "\\", "a\\b",
    "abab", "abab ", "aba", "aa", "aaa", "abcabc", "xabcx", "a\nc", "a%b", "ab\\",
    "é", "aéc", "a€c", "a😀c", "éé", "😀", "é€", "xé€x", "€é€", "aé", "éc", "bab",
    "ab ab", "a b c", "abxab", "xxabxxabxx", "%%", "__", "a_",
]
# binary: '_' is one byte; values need not be UTF-8
LIKE_BIN_PATTERNS = [b"", b"%", b"_", b"a_c", b"a__c", b"%\xff%", b"\xc3_", b"__",
                     b"%_", b"a%c", b"\\%", b"%\x00%"]
LIKE_BIN_VALUES = [b"", b"a", b"abc", b"a\xffc", b"a\xc3\xa9c", b"\xc3\xa9", b"\xff",
                   b"\xff\xfe", b"a\x00c", b"%", b"\x80\x80", b"ac", b"a\xc3c"]


def long_like_cases():
    """(name, pattern, values): long values for the wave shape. The only
    match at the very end; matches that start at 63, 64 and 65 (and across
    the next 64-position step); a middle segment longer than 64 bytes;
    two-byte fillers so that candidate starts skip continuation bytes."""
    out = []
    for n in (1024, 5000):
        vals = ["x" * n, "x" * (n - 3) + "abc", "abc" + "x" * (n - 3),
                "x" * (n - 4) + "abcx", "x" * (n - 2) + "ab"]
        for at in (63, 64, 65, 127, 128, 129, 511, 512, 513):
            vals.append("x" * at + "abc" + "x" * (n - at - 3))
        out.append((f"end-{n}", "%abc", vals))
        out.append((f"mid-{n}", "%abc%", vals))
        out.append((f"start-{n}", "abc%", vals))
        out.append((f"both-{n}", "x%abc%x", vals))
        out.append((f"wild-{n}", "%a_c_", vals))
    needle = "".join(chr(0x41 + i % 26) + chr(0x61 + i % 7) for i in range(35))  # 70
    near = needle[:-1] + "!"
    vals = []
    for at in (0, 63, 64, 65, 200):
        vals.append("y" * at + needle + "y" * 300)
        vals.append("y" * at + near + "y" * 10 + needle)
        vals.append("y" * at + near + "y" * 300)
    out.append(("long-needle", "%" + needle + "%", vals))
    out.append(("long-needle-wild", "%" + needle[:30] + "_" + needle[31:] + "%z", [
        v + "z" for v in vals] + vals))
    # first '%ab%' hit by lane 63 of a step, the second 'ab' right behind it
    vals = ["x" * 63 + "abab" + "x" * 700, "x" * 63 + "aba" + "x" * 700,
            "x" * 62 + "abxab" + "x" * 700, "x" * 127 + "ab" + "x" * 600 + "ab",
            "x" * 127 + "ab" + "x" * 600 + "a"]
    out.append(("two-mids", "%ab%ab%", vals))
    # two-byte code points: every other byte is a continuation byte
    vals = ["é" * 500 + "abc", "é" * 500 + "ab", "é" * 31 + "aéc" + "é" * 600,
            "é" * 32 + "a€c" + "é" * 600, "x" + "é" * 31 + "a😀c" + "é" * 600,
            "é" * 700]
    out.append(("utf8-end", "%_abc", vals))
    out.append(("utf8-mid", "%a_c%", vals))
    out.append(("utf8-count", "%é_a_c_é%", vals))
    return out


def long_cmp_cases():
    """A 1100-byte literal and values that differ from it at the edges of
    the wave compare's 512-byte steps."""
    lit = bytes((i * 37 + 11) & 0xFF for i in range(1100))
    vals = [lit, lit[:-1], lit + b"\x00", lit[:512], lit[:513]]
    for at in (0, 7, 8, 511, 512, 513, 1023, 1024, 1099):
        for d in (1, 0x80):
            vals.append(lit[:at] + bytes([lit[at] ^ d]) + lit[at + 1:])
    vals += [b"", (lit * 5)[:5000], lit * 5]
    return lit, vals
