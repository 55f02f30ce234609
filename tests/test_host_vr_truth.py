"""The host side of native-resolution ground truth (data/vr_ground_truth.py, include/bgnn_vrtruth.h) and of ``Trainer(batch_nodes=)``:
the pair table, the plan of an epoch cut by cell count, the header against its ctypes table, and every refusal of the entry point
without a device.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

from _vr_truth_cpu import assemble_bag, make_pair, native_truth_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, SW = (2.0, 2.0), (1.0, 1.0)


def _grid(h, w, value=10.0):
    return [np.full((h, w), value, np.float32), np.full((h, w), 0.5, np.float32), RES, SW]


def _hand_made():
    """A 2 x 3 base grid with one grid of each kind; the clean file's records in reverse index order."""
    clean = {(0, 0): _grid(2, 3), (0, 1): _grid(4, 4), (1, 0): _grid(3, 5), (1, 2): _grid(2, 2)}
    noisy = {(0, 0): _grid(2, 3), (0, 2): _grid(3, 3), (1, 0): _grid(5, 3), (1, 2): _grid(2, 2)}
    return assemble_bag((2, 3), clean, reverse_records=True), assemble_bag((2, 3), noisy)


# ---- 1. the pair table ------------------------------------------------------------------------------------------------------
def test_pair_table_on_a_hand_made_base_grid():
    from bathymetric_gnn_amd import runtime
    from bathymetric_gnn_amd.data import vr_pair_table
    from bathymetric_gnn_amd.data.vr_ground_truth import PAIRED, UNPAIRED_DIMENSIONS, UNPAIRED_MISSING
    clean, noisy = _hand_made()
    t = vr_pair_table(clean, noisy)
    assert t.rows.dtype == runtime.VT_PAIR_DTYPE and t.total == 6 + 9 + 15 + 4
    assert list(zip(t.base_row.tolist(), t.base_col.tolist())) == [(0, 0), (0, 2), (1, 0), (1, 2)]
    assert t.reason.tolist() == [PAIRED, UNPAIRED_MISSING, UNPAIRED_DIMENSIONS, PAIRED] and t.paired.tolist() == [True, False, False, True]
    assert t.unpaired() == {"missing": 1, "dimensions": 1, "clean_only": 1}                  # (0, 1) exists in the clean file alone
    assert t.rows["out_offset"].tolist() == [0, 6, 15, 30] and t.rows["cells"].tolist() == [6, 9, 15, 4]
    assert t.offsets.tolist() == [0, 6, 15, 30, 34]
    assert t.rows["noisy_start"].tolist() == [0, 6, 15, 30]
    # the clean records lie in reverse order: (1, 2) first, then (1, 0), (0, 1), (0, 0)
    assert t.rows["clean_start"].tolist() == [4 + 15 + 16, -1, -1, 0]
    assert t.hw.tolist() == [[2, 3], [3, 3], [5, 3], [2, 2]] and t.hw.dtype == np.int32
    assert t.res.dtype == np.float64 and t.res.tolist() == [[2.0, 2.0]] * 4
    assert np.isnan(t.clean_res[1:3]).all() and t.clean_res[0].tolist() == [2.0, 2.0]


def test_pair_table_on_the_gpu_tests_fixture_matches_the_restatement():
    from bathymetric_gnn_amd.data import vr_pair_table
    clean, noisy, cases = make_pair("odd")
    t = vr_pair_table(clean, noisy)
    ref = native_truth_cpu(clean, noisy)
    assert list(zip(t.base_row.tolist(), t.base_col.tolist())) == ref["order"]
    assert np.array_equal(t.paired, ref["paired"]) and np.array_equal(t.offsets, ref["offsets"]) and np.array_equal(t.hw, ref["hw"])
    assert np.array_equal(t.res, ref["res"])
    place = {k: i for i, k in enumerate(ref["order"])}
    assert cases["drop_noisy"] not in place and not t.paired[place[cases["drop_clean"]]] and not t.paired[place[cases["transposed"]]]
    assert t.unpaired() == {"missing": 1, "dimensions": 1, "clean_only": 1}
    assert tuple(t.hw[place[cases["big"]]]) == (50, 53)


def test_pair_table_refusals():
    from bathymetric_gnn_amd.data import SRBagHandler, compute_ground_truth_native, vr_pair_table
    clean, noisy = _hand_made()
    other = assemble_bag((3, 2), {(0, 0): _grid(2, 3)})
    with pytest.raises(ValueError, match=r"Base shape mismatch: clean \(3, 2\) vs noisy \(2, 3\)"):
        vr_pair_table(other, noisy)
    short = type(noisy).from_arrays(noisy.varres_metadata, noisy.varres_refinements[:, :-1])
    with pytest.raises(ValueError, match=r"noisy file: the refinement grid at base cell \(1, 2\)"):
        vr_pair_table(clean, short)
    md = clean.varres_metadata.copy()
    md["index"][0, 0] = 40
    with pytest.raises(ValueError, match=r"clean file: the refinement grid at base cell \(0, 0\)"):
        vr_pair_table(type(clean).from_arrays(md, clean.varres_refinements), noisy)
    sr = SRBagHandler.from_arrays(np.zeros((4, 4), np.float32))
    with pytest.raises(TypeError, match="compute_ground_truth"):
        compute_ground_truth_native(sr, sr)


# ---- 2. the plan of an epoch, cut by cell count --------------------------------------------------------------------------------
class _Store:
    """What ``step_plan`` reads of a store: its length and its cell offsets."""

    def __init__(self, cells):
        self.offsets = np.concatenate([[0], np.cumsum(cells)]).astype(np.int64)

    def __len__(self):
        return len(self.offsets) - 1


def _stub_trainer(cells, batch_nodes, seed=5, batch_size=2):
    from bathymetric_gnn_amd.training.trainer import Trainer
    t = Trainer.__new__(Trainer)
    t.seed, t.settings = seed, SimpleNamespace(batch_size=batch_size)
    t.train_store = t.val_store = _Store(cells)
    if batch_nodes != "unset":
        t.batch_nodes = batch_nodes
    return t


def test_step_plan_with_batch_nodes():
    from bathymetric_gnn_amd.training.trainer import dropout_seed
    cells = [9, 100, 2500, 30, 30, 30, 2000, 1, 1999, 25]
    t = _stub_trainer(cells, 2000)
    # validation keeps store order: the greedy cut by hand
    val = t.step_plan(1, validation=True)
    assert [p.tolist() for p, _ in val] == [[0, 1], [2], [3, 4, 5], [6], [7, 8], [9]] and all(s is None for _, s in val)
    # training: the same permutation as without batch_nodes, cut by the same rule; seeds numbered by piece
    order = np.random.default_rng([5, 3]).permutation(len(cells)).tolist()
    plan = t.step_plan(3)
    assert [i for p, _ in plan for i in p.tolist()] == order
    want, run = [[]], 0
    for i in order:
        if want[-1] and run + cells[i] > 2000:
            want.append([]); run = 0
        want[-1].append(i); run += cells[i]
    assert [p.tolist() for p, _ in plan] == want
    assert [s for _, s in plan] == [dropout_seed(5, 3 * len(want) + k) for k in range(len(want))]
    for p, _ in plan:
        assert sum(cells[i] for i in p) <= 2000 or len(p) == 1                 # an oversize tile stands alone
    assert [2] in [p.tolist() for p, _ in plan]
    # a limit no tile reaches: one piece; a limit below every tile: one tile per piece
    assert len(_stub_trainer(cells, 10 ** 9).step_plan(0)) == 1 and len(_stub_trainer(cells, 1).step_plan(0)) == len(cells)


@pytest.mark.parametrize("batch_nodes", [None, "unset"])
def test_step_plan_without_batch_nodes_is_todays(batch_nodes):
    from bathymetric_gnn_amd.training.trainer import dropout_seed
    t = _stub_trainer([5] * 7, batch_nodes)
    order = np.random.default_rng([5, 3]).permutation(7)
    plan = t.step_plan(3)
    assert [p.tolist() for p, _ in plan] == [order[k:k + 2].tolist() for k in range(0, 7, 2)]
    assert [s for _, s in plan] == [dropout_seed(5, 12 + k) for k in range(4)]
    assert [p.tolist() for p, _ in t.step_plan(3, validation=True)] == [[0, 1], [2, 3], [4, 5], [6]]


class _CountedStore(_Store):
    """A store that also carries its tiles' node counts, as every ``TileStore`` constructor leaves them."""

    def __init__(self, cells, nodes):
        super().__init__(cells)
        self.node_counts = np.asarray(nodes, np.int64)


def _counted_trainer(cells, nodes, batch_nodes, seed, batch_size=2):
    t = _stub_trainer(cells, batch_nodes, seed=seed, batch_size=batch_size)
    t.train_store = t.val_store = _CountedStore(cells, nodes)
    return t


# make_pair("odd", lo=1) as TileStore.from_refinement_pairs keeps it: cells and valid cells of its 9 grids
PAIR_CELLS = [45, 12, 2650, 25, 56, 9, 24, 72, 16]
PAIR_NODES = [41, 12, 2644, 23, 1, 9, 23, 71, 16]
ISOLATING = [(1, 1), (8, 0), (19, 1), (31, 2)]        # (seed, epoch) whose cut by 2000 cells leaves tile 4 (one node) alone


def _joined_by_hand(old, nodes):
    """The rule, restated on a list of pieces: a piece below two nodes goes to the piece before it, a first one to the next."""
    out = []
    for p in old:
        if out and sum(nodes[i] for i in p) < 2:
            out[-1] = out[-1] + p
        else:
            out.append(list(p))
    if len(out) > 1 and sum(nodes[i] for i in out[0]) < 2:
        out[1] = out[0] + out[1]
        del out[0]
    return out


def test_the_listed_node_counts_are_the_pairs():
    clean, noisy, _ = make_pair("odd", lo=1)
    ref = native_truth_cpu(clean, noisy)
    keep = ref["paired"] & (ref["grid_counts"][:, 0] >= 1) & (ref["hw"].min(axis=1) >= 2)
    assert np.diff(ref["offsets"])[keep].tolist() == PAIR_CELLS and ref["grid_counts"][keep, 0].tolist() == PAIR_NODES


@pytest.mark.parametrize("seed,epoch", [(s, e) for s in range(40) for e in range(3)])
def test_no_training_step_of_one_node(seed, epoch):
    """Over 40 seeds x 3 epochs: the cut of today isolates the one-node tile at exactly the four listed pairs; the plan never
    does, is still the permutation, and differs from the cut only where a piece was joined to its neighbour."""
    from bathymetric_gnn_amd.training.trainer import dropout_seed
    old = [p.tolist() for p, _ in _stub_trainer(PAIR_CELLS, 2000, seed=seed).step_plan(epoch)]
    t = _counted_trainer(PAIR_CELLS, PAIR_NODES, 2000, seed)
    plan = t.step_plan(epoch)
    new = [p.tolist() for p, _ in plan]
    assert ([4] in old) == ((seed, epoch) in ISOLATING)
    assert all(sum(PAIR_NODES[i] for i in p) >= 2 for p in new)
    assert [i for p in new for i in p] == np.random.default_rng([seed, epoch]).permutation(9).tolist()
    assert all(p.dtype == np.int64 for p, _ in plan)
    assert [s for _, s in plan] == [dropout_seed(seed, epoch * len(new) + k) for k in range(len(new))]
    if (seed, epoch) not in ISOLATING:
        assert new == old
        return
    at = old.index([4])
    if at > 0:                                            # to the piece before it ...
        assert new == old[:at - 1] + [old[at - 1] + [4]] + old[at + 1:]
    else:                                                 # ... a first piece to the one after it
        assert new == [[4] + old[1]] + old[2:]
    assert new == _joined_by_hand(old, PAIR_NODES) and len(new) == len(old) - 1
    # validation keeps the cut: eval() takes one node
    assert [p.tolist() for p, _ in t.step_plan(epoch, validation=True)] == \
        [p.tolist() for p, _ in _stub_trainer(PAIR_CELLS, 2000, seed=seed).step_plan(epoch, validation=True)]


def test_a_first_piece_of_one_node_joins_forward():
    cells, nodes = [56, 1990, 30, 1990, 40], [1, 1900, 30, 1800, 0]
    hit = None
    for seed in range(200):
        t = _counted_trainer(cells, nodes, 2000, seed)
        old = [p.tolist() for p, _ in _stub_trainer(cells, 2000, seed=seed).step_plan(0)]
        new = [p.tolist() for p, _ in t.step_plan(0)]
        assert new == _joined_by_hand(old, nodes) and all(sum(nodes[i] for i in p) >= 2 for p in new)
        if old[0] in ([0], [4], [0, 4], [4, 0]) and hit is None:
            hit = seed
            assert new[0] == old[0] + old[1] and new[1:] == old[2:]
    assert hit is not None
    # a one-node piece in the middle and an empty tile at the end, in store order
    t = _counted_trainer([1990, 56, 1990, 40], [1900, 1, 1800, 0], 2000, 0)
    assert [p.tolist() for p in t._pieces(t.train_store, np.arange(4), trainable=True)] == [[0, 1], [2, 3]]
    assert [p.tolist() for p in t._pieces(t.train_store, np.arange(4))] == [[0], [1], [2], [3]]
    # two pieces below two nodes in a row at the start: together they still cannot train, and go on to the next
    t = _counted_trainer([1990, 1990, 1990], [1, 0, 50], 2000, 0)
    assert [p.tolist() for p in t._pieces(t.train_store, np.arange(3), trainable=True)] == [[0, 1, 2]]


def test_batch_size_rule_with_a_one_node_last_tile():
    cells, nodes = [30] * 7, [20, 20, 20, 20, 20, 20, 1]
    seen = 0
    for seed in range(40):
        t = _counted_trainer(cells, nodes, None, seed, batch_size=2)
        order = np.random.default_rng([seed, 0]).permutation(7).tolist()
        old = [order[k:k + 2] for k in range(0, 7, 2)]
        new = [p.tolist() for p, _ in t.step_plan(0)]
        if order[-1] == 6:
            seen += 1
            assert old[-1] == [6] and new == old[:2] + [old[2] + [6]]
        else:
            assert new == old
    assert seen > 0


def test_a_store_below_two_nodes_is_refused():
    from bathymetric_gnn_amd.training.trainer import Trainer
    with pytest.raises(ValueError, match=r"hold 1 node\(s\) altogether"):
        Trainer(None, None, _CountedStore([56, 9, 16], [1, 0, 0]), batch_nodes=2000)
    with pytest.raises(ValueError, match=r"hold 0 node\(s\) altogether"):
        Trainer(None, None, _CountedStore([56], [0]))


@pytest.mark.parametrize("seed", [0, 1])
def test_training_pair_holds_its_cases(seed):
    """``make_training_pair`` from the input alone: what the GPU tests of the VR training step rely on."""
    from _vr_truth_cpu import TRAINING_RESOLUTIONS, make_training_pair
    clean, noisy, cases = make_training_pair(seed)
    ref = native_truth_cpu(clean, noisy)
    place = {k: i for i, k in enumerate(ref["order"])}
    hw = lambda name: tuple(ref["hw"][place[cases[name]]])
    assert (hw("big"), hw("g22"), hw("g29"), hw("g92"), hw("flat")) == ((24, 31), (2, 2), (2, 9), (9, 2), (7, 7))
    assert ref["grid_counts"][place[cases["sparse"]], 0] == 1 and ref["paired"][place[cases["sparse"]]]
    assert not ref["paired"][place[cases["no_twin"]]] and not ref["paired"][place[cases["transposed"]]]
    assert ref["paired"].sum() == len(ref["order"]) - 2 >= 9
    keep = ref["paired"] & (ref["grid_counts"][:, 0] >= 1) & (ref["hw"].min(axis=1) >= 2)
    assert keep.sum() == ref["paired"].sum()
    want = [TRAINING_RESOLUTIONS[i % 5] for i in range(int(keep.sum()))]
    assert np.array_equal(ref["res"][keep], np.array(want, np.float32).astype(np.float64))
    small = keep.copy(); small[place[cases["big"]]] = False
    assert 100 <= ref["grid_counts"][small, 0].sum() < 256
    big = slice(int(ref["offsets"][place[cases["big"]]]), int(ref["offsets"][place[cases["big"]] + 1]))
    lab = ref["labels"][big]
    assert 0.03 < (lab == 2).mean() < 0.08 and 0.002 < (lab == -1).mean() < 0.03


# ---- 3. the C ABI ------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "bgnn_vrtruth.h")).read()


@pytest.fixture(scope="module")
def lib():
    from bathymetric_gnn_amd import runtime
    if not os.path.exists(runtime.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return runtime.load_library()


def test_vrtruth_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = {name: len([a for a in args.split(",") if a.strip()]) for name, args in re.findall(r"\b(bgnn_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", text)}
    assert sorted(decl) == ["bgnn_vr_ground_truth", "bgnn_vr_ground_truth_workspace_bytes"] == sorted(runtime._VRTRUTH_SIGNATURES)
    for s, n_args in decl.items():
        assert len(runtime._VRTRUTH_SIGNATURES[s][1]) == n_args, s
        assert getattr(lib, s).argtypes == runtime._VRTRUTH_SIGNATURES[s][1] and getattr(lib, s).restype == runtime._VRTRUTH_SIGNATURES[s][0]
    others = [v for k, v in vars(runtime).items() if k.endswith("_SIGNATURES") and k != "_VRTRUTH_SIGNATURES"]
    assert len(others) >= 13 and not any(set(decl) & set(tab) for tab in others)
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_constants_match_the_header():
    from bathymetric_gnn_amd import runtime
    d = {k: int(v) for k, v in re.findall(r"#define\s+(BGNN_[A-Z_0-9]+)\s+(\d+)\b", _header())}
    dt = runtime.VT_PAIR_DTYPE
    assert d["BGNN_VT_PAIR_BYTES"] == dt.itemsize == runtime.VT_PAIR_BYTES == 32
    assert [dt.fields[k][1] for k in ("out_offset", "cells", "noisy_start", "clean_start")] == [0, 8, 16, 24]
    assert d["BGNN_VT_COUNTS"] == runtime.VT_COUNTS == runtime.TILE_COUNTS and d["BGNN_VT_TILE_CELLS"] == runtime.VT_TILE_CELLS
    st = np.dtype(runtime.VT_STATS_DTYPE)
    assert d["BGNN_VT_STATS_BYTES"] == st.itemsize == runtime.VT_STATS_BYTES
    for k in ("valid", "noise", "seafloor", "noise_abs_sum", "noise_abs_median", "noise_abs_max"):
        assert st.fields[k][1] == d["BGNN_VT_STATS_" + k.upper()], k


def test_vrtruth_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    syms = ["bgnn_vr_ground_truth", "bgnn_vr_ground_truth_workspace_bytes"]
    src = tmp_path / "vrtruth_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stddef.h>\n#include <stdio.h>\n#include "bgnn_vrtruth.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = argc < 2 ? 0 : dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (!lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in syms)
                   + '  printf("ok %d %d %d\\n", (int)sizeof(bgnn_vr_pair), BGNN_VT_PAIR_BYTES, (int)offsetof(bgnn_vr_pair, clean_start));\n'
                     "  return 0;\n}\n")
    exe = tmp_path / "vrtruth_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", "32", "32", "24"]


def test_workspace_bytes_is_a_formula(lib):
    ws = lib.bgnn_vr_ground_truth_workspace_bytes
    assert ws(-1, 0) == 0 and ws(0, -1) == 0
    assert ws(1, 1) % 256 == 0 and ws(1, 9) - ws(1, 8) == 256 and ws(1, 8) == ws(1, 1)          # 32 bytes per row, rounded to 256
    assert ws(1024 * 2048, 1) == ws(10 ** 9, 1) > ws(1024 * 1024, 1) > ws(1, 1)                  # 32 bytes per workgroup, at most 2048


def test_hostside_refusals_of_the_call(lib):
    """Every argument check comes before any use of the context or the device.  (The context here is a host buffer: a call that
    touched it, or launched anything, would not come back with these codes.)"""
    from bathymetric_gnn_amd import runtime
    buf = (C.c_int64 * 16384)()
    base = C.addressof(buf) + (-C.addressof(buf)) % 16
    at = lambda off: C.c_void_p(base + off)
    table = lambda *rows: np.array(list(rows), dtype=runtime.VT_PAIR_DTYPE)
    good = table((0, 6, 0, 4), (6, 4, 6, -1))
    need = lib.bgnn_vr_ground_truth_workspace_bytes(10, 2)

    def call(**kw):
        a = {**dict(ctx=at(0), noisy=at(1024), n_noisy=10, clean=at(2048), n_clean=10, pairs=good, n=2, total=10, nodata=1.0e6,
                    thr=0.15, ws=at(16384), ws_bytes=need, labels=at(3072), difference=at(4096), depth=at(5120), unc=at(6144),
                    mask=at(7168), counts=at(8192), stats=at(9216)), **kw}
        p = a["pairs"]
        a["pairs"] = None if p is None else C.c_void_p(p.ctypes.data)
        a["ws_bytes"] = C.c_size_t(a["ws_bytes"])
        return lib.bgnn_vr_ground_truth(*a.values())
    err = lambda: lib.bgnn_last_error()
    assert need + 16384 <= 8 * 16384 - 16
    for name in ("ctx", "noisy", "clean", "pairs", "ws", "labels", "difference", "depth", "mask", "counts", "stats"):
        assert call(**{name: None}) == runtime.ERR_INVALID and b"NULL" in err(), name
    assert call(n_noisy=-1) == runtime.ERR_INVALID and call(n_clean=-1) == runtime.ERR_INVALID and call(n=-1) == runtime.ERR_INVALID
    assert call(total=-1) == runtime.ERR_INVALID
    # a table whose offsets do not tile [0, total)
    assert call(pairs=table((0, 6, 0, 4), (7, 3, 6, -1))) == runtime.ERR_INVALID and b"row 1 of 2" in err() and b"does not continue" in err()
    assert call(pairs=table((1, 6, 0, 4), (7, 3, 6, -1))) == runtime.ERR_INVALID and b"row 0 of 2" in err()
    assert call(total=11) == runtime.ERR_INVALID and b"do not cover" in err()
    assert call(total=9) == runtime.ERR_INVALID and b"row 1 of 2" in err()
    assert call(pairs=table((0, 6, 0, 4), (6, 0, 6, -1)), total=6) == runtime.ERR_INVALID and b"no cell" in err()
    assert call(n=1) == runtime.ERR_INVALID and b"do not cover" in err()
    # record ranges
    assert call(n_clean=9) == runtime.ERR_INVALID and b"leaves the clean records" in err() and b"row 0 of 2" in err()
    assert call(pairs=table((0, 6, 0, 5), (6, 4, 6, -1))) == runtime.ERR_INVALID and b"leaves the clean records" in err()
    assert call(pairs=table((0, 6, 0, -2), (6, 4, 6, -1))) == runtime.ERR_INVALID and b"below -1" in err()
    assert call(n_noisy=9) == runtime.ERR_INVALID and b"leaves the noisy records" in err() and b"row 1 of 2" in err()
    assert call(pairs=table((0, 6, -1, 4), (6, 4, 6, -1))) == runtime.ERR_INVALID and b"leaves the noisy records" in err()
    assert call(pairs=table((0, 6, 2 ** 62, 4), (6, 4, 6, -1))) == runtime.ERR_INVALID and b"leaves the noisy records" in err()
    assert call(clean=None, n_clean=0) == runtime.ERR_INVALID and b"leaves the clean records" in err()
    # workspace and alignment
    assert call(ws_bytes=need - 1) == runtime.ERR_INVALID and b"workspace" in err()
    assert call(ws=at(16392)) == runtime.ERR_INVALID and b"16-byte" in err()
    assert call(noisy=at(1028)) == runtime.ERR_INVALID and b"8-byte" in err()
    assert call(labels=at(3076)) == runtime.ERR_INVALID and call(unc=at(6152)) == runtime.ERR_INVALID and b"16-byte" in err()
    assert call(mask=at(7169)) == runtime.ERR_INVALID and b"mask" in err()
    assert call(counts=at(8196)) == runtime.ERR_INVALID and call(stats=at(9220)) == runtime.ERR_INVALID and b"8-byte" in err()
    assert call(difference=at(1024)) == runtime.ERR_INVALID and b"aliases" in err()
    # nothing to do: whatever the context is, nothing is launched and nothing written
    assert call(n=0, total=0) == 0 and call(n=0, total=0, noisy=None, clean=None, pairs=None, ws=None, labels=None, stats=None) == 0
    assert call(n=2, total=0) == runtime.ERR_INVALID and b"without a cell" in err()
    assert not any(buf)
