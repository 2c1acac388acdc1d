"""Worker of tests/test_fps_paths.py::test_environment_selected_forms: a process of its own because the switches that shape the FPS / k-center chain
(SSDR_KC_TILED, SSDR_FPS_SLOT_SHIFT) are read once per process.  Arguments: "n:na" sizes (D = 32).  For
every size four legs through the C ABI on the gfx950 build — FPS and k-center, over standard-normal rows and over every row twice at shuffled positions —
each printed as "LEG n leg rc status minus match gap_ok forms": entry return code, ssdr_select_status word, picks of -1, picks == oracle (index for
index), input condition met, and the fps_form / fps_seed scopes the profiler reported."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ssdr-al_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from oracle import select_np as O  # noqa: E402
from ssdr_al import _lib  # noqa: E402
from _fps_oracle import make_features, make_seeds, run_abi, trace_fps, trace_kcenter  # noqa: E402

_lib.use(os.path.join(ROOT, "ssdr-al_amd", "libssdr_al.so"))
D, START = 32, 3
for arg in sys.argv[1:]:
    n, na = (int(x) for x in arg.split(":"))
    count = 300 if n <= 5000 else 120
    for kind in ("normal", "ties"):
        f = make_features(kind, n, D, n + 11)
        already = make_seeds("dups", n, na, n)
        for leg in ("fps", "kc"):
            if leg == "fps":
                exp, gap = trace_fps(f, count, START)
                same = np.array_equal(exp, O.farthest_features_sample(f, count, START))
                rc, got, src, st, names = run_abi(f, count, start=START)
            else:
                exp, gap = trace_kcenter(f, already, count)
                # (24 000 x 4000 x 32 doubles do not fit the oracle's one tensor: the replay, which test_replay_equals_the_oracle ties to it, stands alone there)
                same = n * na * D * 8.0 > 2.0e9 or np.array_equal(exp, O.kcenter_greedy(f, already, count))
                rc, got, src, st, names = run_abi(f, count, already=already)
            gap_ok = same and (kind == "ties" or gap >= 1e-9)
            forms = ",".join(sorted(nm for nm in names if nm.startswith(("fps_form:", "fps_seed:")))) or "-"
            print("LEG", n, leg + ("_ties" if kind == "ties" else ""), rc, st, int((got < 0).sum()), int(np.array_equal(got, exp)), int(gap_ok), forms, flush=True)
            if rc != 0 or src != 0 or st != 0:          # a launch that reported a failure: nothing more on the GPU from this process
                sys.exit(0)
