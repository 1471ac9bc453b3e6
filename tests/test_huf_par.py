"""The Huffman-only page classifier (lszstd::huf_only_frame) and the host
twin of the lane-parallel Huffman decode (csrc/cpp/huf_par.h), which runs
the same per-lane steps as the GPU kernel (csrc/hip/zstd_huf.hip).

Corpus (tests/huf_corpus.py): level-1 frames of prefixes of six seeded byte
sources. With libzstd 1.4.8 the classifier accepts all of them except: f64
below 4096 and f32 below 1000 (raw blocks), and int64 < 1e12 at 4096-16384
and uniform 0..15 at 16383 and 16384 (the encoder finds a few matches, so
they carry sequences). The 200-byte entries are single-stream; uniform
0..15 gives equal 4-bit codes with a direct tree description from 256 bytes
on and an FSE-compressed one at 200. The largest maxBits is 11, the format's
limit: min(geometric(0.08) - 1, 255) reaches it from 16383 bytes on, without
sequences."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from lakesoul_amd.ops import cpp

import huf_corpus as hc

LANES = (1, 2, 3, 64, 256)


def _census_says_huf_only(frame: bytes, n: int) -> bool:
    """The same answer from zstd_frame_census, which walks the frame with
    the parse functions: one compressed block (it fails on a second frame
    only by counting its blocks), own-tree Huffman literals, no sequences;
    the literals then hold all n bytes, which the decode tests check."""
    c = cpp().zstd_frame_census(frame)
    blocks = sum(v for k, v in c.items() if k.startswith("block_"))
    lit = sum(v for k, v in c.items() if k.startswith("lit_compressed_"))
    return (blocks == 1 and c.get("block_compressed", 0) == 1 and lit == 1
            and c.get("nseq_zero", 0) == 1 and n <= 131072)


def test_classifier_agrees_with_census():
    raw = 0
    for name, frame, orig in hc.entries():
        got = cpp().zstd_huf_only(frame, len(orig))
        assert got == _census_says_huf_only(frame, len(orig)), name
        if cpp().zstd_frame_census(frame).get("block_raw"):
            raw += 1
            assert not got, name
        # the page's size is part of the question
        assert not cpp().zstd_huf_only(frame, len(orig) + 1), name
    assert raw >= 12  # f64 below 4096 and f32 below 1000
    assert len(hc.accepted()) >= 60


def test_classifier_rejects_sequences_and_multiblock():
    seq = hc.geometric_source(0.35)
    for n in (4096, 65536, 131072):
        frame = cpp().zstd_compress_ref(seq[:n], 1)
        assert cpp().zstd_frame_census(frame).get("nseq_zero", 0) == 0
        assert not cpp().zstd_huf_only(frame, n)
    ids = np.arange(16384, dtype=np.int64).tobytes()
    assert not cpp().zstd_huf_only(cpp().zstd_compress_ref(ids, 1), len(ids))

    from zstd_corpus import corpus

    checked = 0
    for name, comp, orig in corpus():
        c = cpp().zstd_frame_census(comp)
        blocks = sum(v for k, v in c.items() if k.startswith("block_"))
        has_seq = c.get("block_compressed", 0) > c.get("nseq_zero", 0)
        if blocks > 1 or has_seq:
            checked += 1
            assert not cpp().zstd_huf_only(comp, len(orig)), name
    assert checked > 0


def test_corpus_covers_the_format():
    """Every literals size format, stream count and tree description kind
    has an accepted entry; the largest maxBits is recorded and is 11."""
    cen = {name: cpp().zstd_huf_census(frame, len(orig))
           for name, frame, orig in hc.accepted()}
    assert {c["size_format"] for c in cen.values()} == {0, 1, 2, 3}
    # 10-bit sizes are formats 0 (one stream) and 1, 14-bit 2, 18-bit 3
    assert {c["streams"] for c in cen.values()} == {1, 4}
    assert {c["tree"] for c in cen.values()} == {"direct", "fse"}
    for name, c in cen.items():
        if name.endswith("_200"):
            assert c["streams"] == 1, name
    u16 = {c["tree"] for name, c in cen.items() if name.startswith("u16_")}
    assert u16 == {"direct", "fse"}
    assert all(c["max_bits"] == 4 for name, c in cen.items()
               if name.startswith("u16_") and not name.endswith("_200"))
    largest = max(c["max_bits"] for c in cen.values())
    print("largest maxBits:", largest)
    assert largest == 11
    # and between 0.08 and 0.35, still without sequences
    for p in (0.1, 0.12, 0.15):
        data = hc.geometric_source(p)[:65536]
        frame = cpp().zstd_compress_ref(data, 1)
        assert cpp().zstd_huf_only(frame, len(data))
        assert cpp().zstd_huf_census(frame, len(data))["max_bits"] == 11


@pytest.mark.parametrize("lanes", LANES)
def test_par_decode_equals_original(lanes):
    for name, frame, orig in hc.accepted():
        out, _ = cpp().zstd_huf_par_decode_ref(frame, lanes, len(orig))
        assert out == orig, (name, lanes)


def test_equal_length_codes_take_the_slow_path():
    """Equal 4-bit codes never resynchronise: where the cuts fall inside a
    codeword, lane k is only right after round k."""
    rounds = {}
    for name, frame, orig in hc.accepted():
        if name.startswith("u16_") and not name.endswith("_200"):
            out, r = cpp().zstd_huf_par_decode_ref(frame, 64, len(orig))
            assert out == orig
            rounds[name] = r
    print("fix-up rounds at 64 lanes:", rounds)
    assert max(rounds.values()) > 2
    assert rounds["u16_1025"] == 63
    # real column bytes: one or two rounds on a full page
    for name in ("f64_131072", "f32_131072", "i64_131072"):
        frame, orig = next((f, o) for n, f, o in hc.accepted() if n == name)
        assert cpp().zstd_huf_par_decode_ref(frame, 64, len(orig))[1] <= 2


def test_damaged_frames_fail_cleanly():
    """Truncated frames and frames with one flipped byte in the tree or a
    stream either fail or decode to exactly len(orig) bytes; the sanitizer
    program checks that nothing is touched outside the destination."""
    rng = np.random.default_rng(21)
    failed = 0
    for name, frame, orig in hc.accepted():
        if len(orig) > 4096:
            continue
        for cut in (1, 2, len(frame) // 2):
            out, _ = cpp().zstd_huf_par_decode_ref(frame[:-cut], 64, len(orig))
            assert out is None, (name, cut)
        for _ in range(24):
            i = int(rng.integers(9, len(frame)))
            bad = bytearray(frame)
            bad[i] ^= 1 << int(rng.integers(0, 8))
            out, _ = cpp().zstd_huf_par_decode_ref(bytes(bad), 64, len(orig))
            assert out is None or len(out) == len(orig)
            failed += out is None
    assert failed > 0


def test_huf_par_sanitizer_clean(tmp_path):
    """Classifier and host twin under AddressSanitizer + UBSan on every
    accepted frame and a few hundred one-byte corruptions of each, input
    and output in exactly-sized heap buffers
    (csrc/cpp/tests/huf_par_san.cc)."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "csrc", "cpp", "tests", "huf_par_san.cc")
    exe = str(tmp_path / "huf_par_san")
    cc = shutil.which("g++")
    if cc is None:
        pytest.skip("no g++")
    b = subprocess.run([cc, "-O1", "-g", "-std=c++17",
                        "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", src, "-o", exe,
                        "-l:libzstd.so.1"], capture_output=True, text=True)
    if b.returncode != 0:
        pytest.skip(f"sanitizer build unavailable: {b.stderr[-200:]}")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, \
        r.stderr[:4000]
