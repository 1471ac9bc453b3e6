"""GPU decode of Huffman-only zstd pages (csrc/hip/zstd_huf.hip): the kernel
against the original bytes, the old kernel and (through tests/test_huf_par.py,
same corpus) its host twin; and the scan route that feeds it."""

import numpy as np
import pytest
import torch

from lakesoul_amd.ops import cpp, hip

import huf_corpus as hc

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests require an MI355X"
    return torch.device("cuda:0")


def test_huf_kernel_decodes_corpus(dev):
    """Every accepted corpus frame as one jobs table in one launch: 1 and 4
    streams, all literals size formats, direct and FSE tree descriptions,
    maxBits 4 to 11, equal-length codes that need all 255 fix-up rounds,
    outputs from 200 bytes to 128 KB at odd offsets. 64 guard bytes between
    the pages stay intact."""
    entries = hc.accepted()
    assert len(entries) >= 60
    src = b"".join(f for _, f, _ in entries)
    jobs, soff, doff = [], 0, GUARD
    for _, frame, orig in entries:
        jobs.append([soff, len(frame), doff, len(orig)])
        soff += len(frame)
        doff += len(orig) + GUARD
    expect = np.full(doff, 0xA5, dtype=np.uint8)
    for (_, _, orig), j in zip(entries, jobs):
        expect[j[2]:j[2] + j[3]] = np.frombuffer(orig, dtype=np.uint8)
    src_d = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).to(dev)
    jobs_d = torch.tensor(jobs, dtype=torch.int64, device=dev)
    dst = torch.full((doff,), 0xA5, dtype=torch.uint8, device=dev)
    status = hip().zstd_huf_decompress_into(src_d, jobs_d, dst)
    assert status.cpu().tolist() == [0] * len(entries)
    got = dst.cpu().numpy()
    for (name, _, _), j in zip(entries, jobs):
        assert np.array_equal(got[j[2]:j[2] + j[3]], expect[j[2]:j[2] + j[3]]), name
        assert (got[j[2] - GUARD:j[2]] == 0xA5).all(), f"guard before {name}"
    assert (got[-GUARD:] == 0xA5).all()
    assert np.array_equal(got, expect)

    # the general zstd kernel agrees
    dst2 = torch.full((doff,), 0xA5, dtype=torch.uint8, device=dev)
    status2 = hip().zstd_decompress_into(src_d, jobs_d, dst2)
    assert int((status2 != 0).sum()) == 0
    assert torch.equal(dst, dst2)


def _mk_catalog(tmp_path):
    from lakesoul_amd.meta.client import MetaClient
    from lakesoul_amd.meta.store import SqliteMetaStore
    from lakesoul_amd.tables.catalog import LakeSoulCatalog

    store = SqliteMetaStore(str(tmp_path / "meta.db"))
    return LakeSoulCatalog(MetaClient(store), warehouse=str(tmp_path / "wh"))


def test_huf_scan_route(dev, tmp_path, monkeypatch):
    """Merge-on-read scan of id int64, v float64, f float32, t int64: the
    v, f and t pages are Huffman jobs, the sorted id pages (sequences) are
    not; the GPU scan equals the CPU scan with the route on and off."""
    import pandas as pd

    import lakesoul_amd.io.reader_gpu as rgpu
    from lakesoul_amd.io.schema import Field, Schema

    # several pages per chunk (when this process has not written a file
    # yet: the writer reads the variable once; 2 per v and t chunk if not)
    monkeypatch.setenv("LAKESOUL_PAGE_BYTES", "65536")
    t = _mk_catalog(tmp_path).create_table(
        "huf",
        Schema([Field("id", "int64", False), Field("v", "float64", False),
                Field("f", "float32", False), Field("t", "int64", False)]),
        primary_keys=["id"],
        hash_bucket_num=2,
    )
    rng = np.random.default_rng(31)

    def rows(ids):
        n = len(ids)
        return {"id": ids.astype(np.int64), "v": rng.normal(size=n),
                "f": rng.normal(size=n).astype(np.float32),
                "t": rng.integers(0, 10 ** 12, n).astype(np.int64)}

    n = 40000
    t.upsert(rows(np.arange(n)))
    t.upsert(rows(np.arange(0, n, 2)))
    t.upsert(rows(np.arange(1, n, 3)))
    names = ["id", "v", "f", "t"]
    cpu_df = (t.scan(device="cpu").to_arrow().to_pandas()
              .sort_values("id").reset_index(drop=True))
    assert len(cpu_df) == n

    for on in (True, False):
        monkeypatch.setattr(rgpu, "_GPU_HUF", on)
        njobs = {c: 0 for c in names}
        units = t.scan(device="cuda").plan()
        assert len(units) == 2 and all(len(u.files) == 3 for u in units)
        for u in units:
            raw = rgpu.fetch_raw(u.files, names)
            jobs = raw["huf_jobs"].view(-1, 4)
            desc = raw["desc"]
            for dst_off in jobs[:, 2].tolist():
                for row in range(desc.shape[0]):
                    a = int(desc[row, cpp().UD_VAL_OFF])
                    if a <= dst_off < a + int(desc[row, cpp().UD_VAL_LEN]):
                        njobs[names[row % len(names)]] += 1
        if on:
            assert njobs["id"] == 0 and min(njobs[c] for c in "vft") > 0, njobs
            assert njobs["v"] > len(t.files()), "several pages per chunk"
        else:
            assert sum(njobs.values()) == 0, njobs
        gpu_df = (t.scan(device="cuda").to_arrow().to_pandas()
                  .sort_values("id").reset_index(drop=True))
        pd.testing.assert_frame_equal(cpu_df, gpu_df)
