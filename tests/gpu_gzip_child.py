"""Child process of test_gpu_gzip.py: scans a table on the GPU through the
production reader, which takes LAKESOUL_GPU_GZIP from the environment at
import.

    python gpu_gzip_child.py OUT_DIR META_DB WAREHOUSE TABLE

Writes OUT_DIR/scan.arrow (the scan, Arrow IPC) and OUT_DIR/jobs.json: the
(compressed, uncompressed) sizes of every gzip job of every unit that
fetch_raw read."""

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pyarrow as pa  # noqa: E402


def main():
    out, meta_db, warehouse, name = sys.argv[1:5]
    from lakesoul_amd.io import reader_gpu
    from lakesoul_amd.meta.client import MetaClient
    from lakesoul_amd.meta.store import SqliteMetaStore
    from lakesoul_amd.tables.catalog import LakeSoulCatalog

    jobs = []
    real = reader_gpu.fetch_raw

    def spy(files, names):
        raw = real(files, names)
        jobs.extend(raw["gzip_jobs"].view(-1, 4)[:, [1, 3]].tolist())
        return raw

    reader_gpu.fetch_raw = spy
    catalog = LakeSoulCatalog(MetaClient(SqliteMetaStore(meta_db)),
                              warehouse=warehouse)
    tbl = catalog.table(name).scan(device="cuda").to_arrow()
    with pa.OSFile(os.path.join(out, "scan.arrow"), "wb") as f:
        with pa.ipc.new_file(f, tbl.schema) as w:
            w.write_table(tbl)
    with open(os.path.join(out, "jobs.json"), "w") as f:
        json.dump({"flag": reader_gpu._GPU_GZIP, "jobs": jobs}, f)


if __name__ == "__main__":
    main()
