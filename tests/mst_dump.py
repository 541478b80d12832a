"""Test infrastructure: `python tests/mst_dump.py OUT_DIR SHAPE:MODE [SHAPE:MODE ...]` builds each named set of
mst_shapes.py, runs lcsgpu_mst_prim (kind 1) on it under LCSGPU_MST_MODE=MODE and writes the edges as float64 rows
(from, to, dist) to OUT_DIR/SHAPE_MODE.npy.  Started as a process of its own wherever a switch is read only once per
process (LCSGPU_TUNE, taken from the environment as it is)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import famsa_amd  # noqa: E402
import mst_shapes  # noqa: E402


def main(out_dir, jobs):
    eng = famsa_amd.LcsGpu(0)
    try:
        uploaded = None
        for job in jobs:
            name, mode = job.split(":")
            if name != uploaded:
                eng.upload_seqs(mst_shapes.build(name))
                uploaded = name
            os.environ["LCSGPU_MST_MODE"] = mode
            e = eng.mst_prim(1)
            np.save(os.path.join(out_dir, "%s_%s.npy" % (name, mode)),
                    np.stack([e["from"].astype(np.float64), e["to"].astype(np.float64), e["dist"]], axis=1))
    finally:
        eng.close()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
