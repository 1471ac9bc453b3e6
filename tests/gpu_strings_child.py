"""Child process of test_gpu_strings.py: scans tables on the GPU through the
production reader, which takes LAKESOUL_GPU_STRINGS from the environment at
import.

    python gpu_strings_child.py OUT_DIR META_DB WAREHOUSE TABLE[,TABLE...]

Writes OUT_DIR/TABLE.arrow (the scan, Arrow IPC) per table and
OUT_DIR/tags.json: per table, the UD_STR column of every unit that
fetch_raw read."""

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pyarrow as pa  # noqa: E402


def main():
    out, meta_db, warehouse, tables = (sys.argv[1], sys.argv[2], sys.argv[3],
                                       sys.argv[4].split(","))
    from lakesoul_amd.io import reader_gpu
    from lakesoul_amd.meta.client import MetaClient
    from lakesoul_amd.meta.store import SqliteMetaStore
    from lakesoul_amd.ops import cpp
    from lakesoul_amd.tables.catalog import LakeSoulCatalog

    seen = []
    real = reader_gpu.fetch_raw

    def spy(files, names):
        raw = real(files, names)
        seen.append(raw["desc"][:, cpp().UD_STR].tolist())
        return raw

    reader_gpu.fetch_raw = spy
    catalog = LakeSoulCatalog(MetaClient(SqliteMetaStore(meta_db)),
                              warehouse=warehouse)
    tags = {}
    for name in tables:
        del seen[:]
        tbl = catalog.table(name).scan(device="cuda").to_arrow()
        with pa.OSFile(os.path.join(out, f"{name}.arrow"), "wb") as f:
            with pa.ipc.new_file(f, tbl.schema) as w:
                w.write_table(tbl)
        tags[name] = [list(t) for t in seen]
    with open(os.path.join(out, "tags.json"), "w") as f:
        json.dump(tags, f)


if __name__ == "__main__":
    main()
