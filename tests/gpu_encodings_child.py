"""Child process of test_gpu_encodings.py::test_env_forces_host_route: reads
one unit through the production reader (reader_gpu.fetch_raw, which takes
its routes from the environment at import) and decodes it on the GPU.

    python gpu_encodings_child.py OUT.npz NAME[,NAME...] FILE [FILE...]

Writes the descriptor's encoding tags and, per unit column, its bytes and
validity."""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    out, names, files = sys.argv[1], sys.argv[2].split(","), sys.argv[3:]
    from lakesoul_amd.io.reader_gpu import UnitTransfer, fetch_raw
    from lakesoul_amd.ops import cpp, hip

    dev = torch.device("cuda:0")
    raw = fetch_raw(files, names)
    tr = UnitTransfer(raw, dev)
    e_u8 = torch.empty(0, dtype=torch.uint8, device=dev)
    e_i64 = torch.empty(0, dtype=torch.int64, device=dev)
    outs = hip().decode_unit(
        tr.vals, tr.validity if tr.validity is not None else e_u8,
        tr.dicts if tr.dicts is not None else e_u8,
        tr.runs if tr.runs is not None else e_i64,
        tr.soffs if tr.soffs is not None else e_i64, raw["desc"],
        len(files), len(names), tr.enc)
    res = {"enc": raw["desc"][:, cpp().UD_ENC].numpy()}
    for u, entry in enumerate(outs):
        data, valid = entry
        res[f"data{u}"] = data.cpu().numpy()
        res[f"valid{u}"] = (valid.cpu().numpy() if valid is not None
                            else np.zeros(0, dtype=np.uint8))
    np.savez(out, **res)


if __name__ == "__main__":
    main()
