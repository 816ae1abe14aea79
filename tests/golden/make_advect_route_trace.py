"""Record ``tests/golden/advect_route_trace.txt``: what the advect dispatcher asked of the HIP runtime, and which kernel it
reported, at the commit BEFORE its launch ladders were built by one helper (``tests/c/advect_route_trace.cpp`` holds the
cases, ``tests/c/fake_hip.c`` the recording runtime).

    git checkout <parent> -- lagrangiancoherence_amd/csrc && python tests/golden/make_advect_route_trace.py <parent>

The file is the parent's behaviour and is not regenerated from later code.  Per group of cases (environment, call, dtype,
x boundary): the SHA-256 of the cases' traces, the count of each kind of line and the number of cases (the traces themselves
come to some 70 MB).  Runs on the CPU in seconds; two runs give the same bytes."""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import test_advect_route_trace as T  # noqa: E402

if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:
        cases = T.H.run_driver(T.H.build_driver(tmp, "advect_route_trace"))
    missing = [n for n in T.KR.ROUTES if not n.startswith("sigma") and n not in T.UNREACHED_ON_CPU and n not in T.reported(cases)]
    assert not missing, missing          # the parent alone satisfies the coverage test
    with open(T.GOLDEN, "w") as f:
        f.write(f"# recorded at {sys.argv[1]}\n# <group> || <sha256 of its cases' traces> <lines of each kind> <cases>\n")
        for group, digest in T.record(cases).items():
            f.write(f"{group} || {digest}\n")
    print(len(cases), "cases,", sum(len(c) for c in cases.values()), "trace lines")
