"""The packed model's layout and host packers (csrc/model_images.h) without a GPU: tests/pack_host_check.cpp is compiled from that
header alone, run, and its JSON document compared with tests/golden/pack_images.json.

Where the golden values come from.  Totals, `HT`, `htab_ok`, `f16_ok`, the float16 scales, the hash of the filled blob (and of the
zero-padded weight blob), every image's OFFSET, and the refresh tables (their sizes, the fold offsets, a hash of each table with
its entries sorted) are those of the packer as it stood BEFORE the image table existed (commit 51238b7, `Packed::pack` /
`Packed::assign` / `model_refresh_tables` in csrc/model_pack.hip), not of the code under test.  Recipe: a scratch program that
`#include`s that commit's model_pack.hip after mapping hipSetDevice / hipMalloc / hipMemcpy / hipFree onto their host
counterparts with four `#define`s, adds a one-line `bgnn::set_error`, carries the same case list and weight generator as
pack_host_check.cpp, and prints `Packed`'s `o_*` / `lo[]` fields and the tables `model_create_native` + `model_refresh_tables`
leave; compiled with `hipcc --offload-arch=gfx950 -x hip`, run on the CPU.  Only what that packer never recorded comes from
model_images.h itself -- each image's `floats` and flags, the hash of `h_V` -- and this file checks those on their own: the images
tile the blob exactly, the TRAIN set is listed below by hand, every COPY flag is probed, and the refresh plan is checked as a
property (fill from weights A, apply the plan with weights B: TRAIN images are B's byte for byte, all others still A's)."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "pack_images.json")))
PROPERTY_CASES = ["gat_default", "gat_128x4", "gat_one_layer", "sage_64", "gin_64"]


def _cxx():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (shutil.which("g++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), shutil.which("amdclang++"), shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no C++ compiler: neither g++ nor ROCm's clang++")


@pytest.fixture(scope="module")
def doc(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pack") / "pack_host_check"
    subprocess.run([_cxx(), "-std=c++17", "-O1", os.path.join(ROOT, "tests", "pack_host_check.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def test_case_list(doc):
    assert sorted(doc) == sorted(GOLDEN) and len(doc) == 15


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_pack_is_the_parent_packers(doc, case):
    got, want = doc[case], GOLDEN[case]
    for key in sorted(set(got) | set(want)):
        assert got.get(key) == want.get(key), f"{case}: {key}"


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_images_tile_the_blob(doc, case):
    at = 0
    for name, (off, floats, _) in sorted(doc[case]["images"].items(), key=lambda kv: kv[1][0]):
        assert off == at and floats > 0, name
        at += (floats + 3) // 4 * 4
    assert at == doc[case]["total"]


COMMON = {("fe_W0t", "TC"), ("fe_b0", "TC"), ("fe_W1t", "TC"), ("fe_b1", "TC"), ("tr_bias", "TC"), ("bn_w", "TC"), ("bn_b", "TC"),
          ("hd_W0", "TC"), ("hd_W0t", "TC"), ("hd_b0", "TC"), ("hd_W1", "TC"), ("hd_b1", "TC")}
GAT = COMMON | {("Wt", "TC"), ("att_src", "TC"), ("att_dst", "TC"), ("V", "T"), ("l0f_Wt", "T"), ("l0f_b", "T")}
TRAIN_SETS = {
    "gat_default": GAT | {("l0f_Wpm", "TR")},
    "gat_two_heads_in7": GAT | {("l0f_Wpm", "TR")},
    "gat_128x4": GAT | {("l0f_Wpm", "TR"), ("Wt_blk", "TC"), ("l0f_Wt_blk", "TR")},
    "gat_64x8": GAT | {("l0f_Wpm", "TR"), ("Wt_blk", "TC"), ("l0f_Wt_blk", "TR")},
    "gat_one_layer": GAT | {("l0f_Wpm", "TR")},
    "gat_32x2_edge1": GAT | {("l0f_Wpm", "TR")},
    "gat_32x1_16cls": GAT,
    "gcn_64": COMMON | {("Wt", "TC")},
    "sage_64": COMMON | {("tr_Wt", "TC")},
    "gin_64": COMMON | {("Wt", "TC"), ("b1", "TC"), ("tr_Wt", "TC")},
    "gcn_32": COMMON | {("Wt", "TC")},
    "sage_128": COMMON | {("tr_Wt", "TC")},
    "gin_32": COMMON | {("Wt", "TC"), ("b1", "TC"), ("tr_Wt", "TC")},
    "gat_default_beyond_f16": GAT | {("l0f_Wpm", "TR")},
    "gat_48x3_padded": GAT | {("l0f_Wpm", "TR")},
}


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_train_set_is_what_training_reads(doc, case):
    got = {(name.split(".")[-1], flags) for name, (_, _, flags) in doc[case]["images"].items() if "T" in flags}
    assert got == TRAIN_SETS[case]
    assert doc[case]["copy_flags_hold"] is True
    assert doc[case]["plan"]["error"] == ""


@pytest.mark.parametrize("case", PROPERTY_CASES)
def test_refresh_plan_property(doc, case):
    assert doc[case]["plan_property"] == "ok"


def test_shape_dependent_images(doc):
    """which images exist for which shape, and the value-dependent results of the case beyond float16's range"""
    im = {c: set(doc[c]["images"]) for c in doc}
    assert {"l0af_W", "l0af_shift"} <= im["gat_default"] and "l0af_W" not in im["gat_128x4"] and "l0af_W" not in im["gat_64x8"]
    assert "l0f_Wt_blk" in im["gat_128x4"] and "L0.Wt_blk" in im["gat_64x8"] and "L2.Wt_blk" not in im["gat_64x8"]
    assert "l0f_Wt_blk" not in im["gat_default"] and "L0.Wt_blk" not in im["gat_default"]
    assert "l0f_Wpm" not in im["gat_32x1_16cls"] and "l0f_Wpm" in im["gat_32x2_edge1"]
    assert all("hd_tab" in im[c] for c in doc)
    assert [c for c in sorted(doc) if not doc[c]["htab_ok"]] == ["gat_128x4", "gat_32x1_16cls", "gat_32x2_edge1", "gcn_32", "gin_32", "sage_128"]
    for c in ("gcn_64", "sage_64", "gin_64"):
        assert "L0.Wfp" in im[c] and "l0f_Wt" in im[c] and "hd_W0sp" not in im[c]
    for c in ("gcn_32", "sage_128", "gin_32"):
        assert "L0.Wfp" not in im[c]
    assert [c for c in doc if not doc[c]["f16_ok"]] == ["gat_default_beyond_f16"]
    assert doc["gat_default_beyond_f16"]["inv16"][1] == 1.0 and doc["gat_default"]["inv16"][1] < 1.0
    assert doc["gat_48x3_padded"]["padded_weights"] == doc["gat_default"]["weights"]
