"""Worker of tests/test_graph_paths.py::test_slices_switch: a process of its own because SSDR_CHAMFER_SLICES (csrc/select_chamfer.hip: chamfer_slices) is
static and read once per process.  Argument: the library to bind (the gfx950 build or the CPU logic build).  Every input (tests/_graph_paths.py) goes through
ssdr_cloud_graph_batch_dev in float64 mode with gcn_top = 3 and is printed as "DIGEST name sha256-of-dir" and "CASE name ok"; the process stops at the first
call that fails."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ssdr-al_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from ssdr_al import _lib  # noqa: E402
import _graph_paths as G  # noqa: E402

_lib.use(sys.argv[1])
G.set_chamfer_mode("f64")
for name, clouds in (("batch", G.batch_clouds()),):
    try:
        got = G.graph_batch(clouds, gcn_top=3)
    except Exception as e:          # a launch that reported a failure: nothing more on the device from this process
        print("CASE", name, "failed:", e, flush=True)
        sys.exit(0)
    print("DIGEST", name, hashlib.sha256(b"".join(np.ascontiguousarray(g[1]).tobytes() for g in got)).hexdigest(), flush=True)
    print("CASE", name, "ok", flush=True)
