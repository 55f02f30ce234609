"""The layout of a tile batch (csrc/graph_plan.h) without a GPU: tests/graph_plan_check.cpp is compiled from that header alone, run,
and its JSON document compared with tests/golden/graph_plan.json.

Where the golden values come from.  Every value in the golden file is what `graph_build_impl` in csrc/bgnn_api.hip computed BEFORE the
planner existed (commit 3ba8673), not what the header under test gives.  Recipe: a scratch program that `#include`s that commit's
bgnn_api.hip after mapping hipSetDevice / hipMalloc / hipFree / hipHostMalloc / hipEventCreateWithFlags / hipEventRecord /
hipEventQuery / hipMemcpyAsync / hipStreamSynchronize / hipGetLastError onto host counterparts with `#define`s (malloc, memcpy,
hipSuccess), carries the case list of graph_plan_check.cpp, and defines `bgnn::launch_graph_build` as a stub that prints the handle's
fields and hashes the tables the build "uploaded" (the two cached tables of a uniform batch; the one block of a ragged batch up to the
end of its last table, its offsets as pointer differences, its allocation as the pool's size of the block).  Each case runs
`bgnn_graph_build` on a fresh `bgnn_ctx` (num_cus and ragged_atlas set by hand, no device behind it); the error cases record the
return code and `bgnn_last_error()`.  Compiled with `hipcc --offload-arch=gfx950 -x hip -Wl,--unresolved-symbols=ignore-all`, run on
the CPU.  `item_cells` was a local of that function: it is recorded where the handle kept it, in the table-cache key of the cacheable
cases; for the others the row-band count and the block hash pin it.  "props" is not a golden value: the checker works the plan's
invariants out on its own (bands and block lists cover each tile once, the block's offsets, the canvas), and "ok" is asserted below.

Cases beyond the issue's list: `32x64_64cus`, whose item_cells (512) lies strictly between the clamps -- 128 tiles of 64x64 on 64 CUs
come to exactly the upper clamp."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "graph_plan.json")))
RAGGED = ["vr65_k8", "vr65_k16", "vr65_k8_no_atlas", "vr65_k16_no_atlas", "many420_k8", "many420_k16", "rejected_canvas",
          "single_candidate"]


def _cxx():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (shutil.which("g++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), shutil.which("amdclang++"), shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no C++ compiler: neither g++ nor ROCm's clang++")


@pytest.fixture(scope="module")
def doc(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan") / "graph_plan_check"
    subprocess.run([_cxx(), "-std=c++17", "-O1", os.path.join(ROOT, "tests", "graph_plan_check.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_case_list(doc):
    assert sorted(doc) == sorted(GOLDEN) and len(doc) == 17


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_plan_is_the_parent_builds(doc, case):
    got, want = doc[case], GOLDEN[case]
    for key in sorted(set(got) | set(want)):
        assert got.get(key) == want.get(key), f"{case}: {key}"


@pytest.mark.parametrize("case", sorted(c for c in GOLDEN if GOLDEN[c]["error"] == 0))
def test_plan_properties(doc, case):
    assert doc[case]["props"] == "ok"


def test_what_the_cases_pin(doc):
    """each case reaches the branch it is there for"""
    assert doc["one_256"]["key"][3] == 256 and doc["headline_128x256"]["key"][3] == 2048        # the item_cells clamps ...
    assert doc["128x64_64cus"]["key"][3] == 2048 and doc["32x64_64cus"]["key"][3] == 512        # ... and between them
    assert doc["one_2x2"]["blocks2"] == [1, 1, 1] and doc["one_2x2"]["n_items"] == 1
    assert doc["three_181x199"]["blocks2"] == [12, 13, 468] and doc["three_181x199"]["blocks3"] == [23, 13, 897]
    two = doc["two_64_two_resolutions"]
    assert two["uniform"] == 1 and two["cacheable"] == 0 and "key" not in two
    for c in RAGGED:
        assert doc[c]["uniform"] == 0 and doc[c]["cacheable"] == 0 and doc[c]["block_alloc"] % 256 == 0
    # the ordinary VR batch: 456 canvas blocks against 496 per-grid blocks; the 16-dilated stencil's gutter of 2 costs two block rows
    assert doc["vr65_k8"]["atlas"] == [304, 192] and doc["vr65_k16"]["atlas"] == [304, 208] and doc["vr65_k8"]["blocks3"][2] == 496
    for c in ("vr65_k8_no_atlas", "vr65_k16_no_atlas", "rejected_canvas"):                     # no canvas: the items3 table travels
        assert doc[c]["atlas"] == [0, 0] and doc[c]["offsets"][3] > 0 and doc[c]["offsets"][4:] == [0, 0]
    for c in ("vr65_k8", "vr65_k16", "many420_k8", "many420_k16", "single_candidate"):          # a canvas: its two tables instead
        assert doc[c]["atlas"][1] > 0 and doc[c]["offsets"][3] == 0 and doc[c]["offsets"][4] > 0 and doc[c]["offsets"][5] > 0
    assert doc["rejected_canvas"]["blocks3"][2] == 35                                            # (its canvas would have had 50)
    assert doc["single_candidate"]["atlas"] == [304, 8]
    assert doc["error_1x5"]["error"] == -1 and doc["error_1x5"]["message"].startswith("Shape of array too small to calculate a numerical gradient")
    assert doc["error_1x5"]["message"].endswith("(tile 0 is 1x5)")
    assert doc["error_2pow30"] == {"error": -1, "message": "batch too large: 2^30 cells or more; split it"}
