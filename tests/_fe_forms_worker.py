"""Worker of tests/test_subsample_paths.py::test_environment_selected_forms: a process of its own because the switches that select a form of the bucket
partition (SSDR_FE_WGS, SSDR_FE_MOVE_WGS; csrc/frontend.hip) are static and read once per process.  Arguments: the library to bind (the gfx950
build or the CPU logic build) and the group of inputs (tests/_fe_paths.py: form_inputs).  Every input goes through ssdr_grid_subsample_batch_dev under
SSDR_SUBSAMPLE_AUTO and under SSDR_SUBSAMPLE_SORT, each printed as "CASE name rc status match": return code of ssdr_grid_subsample_status, its status word,
and whether the rows of the clouds that must match equal the oracle's bit for bit.  The input conditions are asserted before the library is called."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ssdr-al_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import oracle  # noqa: E402
from ssdr_al import _lib  # noqa: E402
from _fe_paths import AUTO, SORT, form_inputs, oracle_rows, rows_equal, run_batch  # noqa: E402

_lib.use(sys.argv[1])
orc = oracle.c()
for name, clouds, dl, auto_status, auto_match in form_inputs(sys.argv[2]):
    exp = [oracle_rows(orc, c, dl) for c in clouds]
    for method, tag, want, which in ((AUTO, "auto", auto_status, auto_match), (SORT, "sort", 0, tuple(range(len(clouds))))):
        rc, st, rows = run_batch(clouds, dl, method)
        print("CASE", "%s/%s" % (name, tag), rc, st, int(all(rows_equal(rows[r], exp[r]) for r in which)), flush=True)
        if st != want or (rc != 0) != (want != 0):          # a launch that reported a failure: nothing more on the device from this process
            sys.exit(0)
