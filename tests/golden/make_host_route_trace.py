"""Record ``tests/golden/host_route_trace.txt``: what ``lc_lcs_host``, ``lc_lcs_global_host`` and the positional ``lc_advect``
entry points asked of the HIP runtime at the commit BEFORE the two host routes got one device-side core
(``tests/c/host_route_trace.cpp`` holds the calls, ``tests/c/fake_hip.c`` the recording runtime).

    git checkout <parent> -- lagrangiancoherence_amd/csrc && python tests/golden/make_host_route_trace.py <parent>

The file is the parent's behaviour and is not regenerated from later code.  Per call: its label, the SHA-256 of its trace and
the count of each kind of line (the traces themselves come to some 640 KB).  Runs on the CPU in seconds; two runs give the
same bytes."""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import test_host_route_trace as T  # noqa: E402

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        calls = T.run_driver(T.build_driver(tmp))
    with open(T.GOLDEN, "w") as f:
        f.write(f"# recorded at {sys.argv[1]}\n# <call> | <sha256 of its trace> <lines of each kind>\n")
        for label, lines in calls.items():
            f.write(f"{label} | {T.summary(lines)}\n")
    print(len(calls), "calls,", sum(len(c) for c in calls.values()), "trace lines")
