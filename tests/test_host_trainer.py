"""The host side of the Trainer (training/trainer.py, include/bgnn_trainer.h): the header against its ctypes table, the early-stopping
rule, the training-settings accessor, the ground-truth tile scan and what the ``training`` package exports.  No GPU needed."""
import ctypes as C
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bgnn_trainer.h")).read(), flags=re.S)


def _declarations():
    """{symbol: number of arguments} of every function bgnn_trainer.h declares."""
    out = {}
    for name, args in re.findall(r"\b(bgnn_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", _header()):
        out[name] = len([a for a in args.split(",") if a.strip()])
    return out


@pytest.fixture(scope="module")
def lib():
    from bathymetric_gnn_amd import runtime
    if not os.path.exists(runtime.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return runtime.load_library()


def test_trainer_symbols_exported_and_bound(lib):
    from bathymetric_gnn_amd import runtime
    decl = _declarations()
    assert sorted(decl) == ["bgnn_epoch_accumulate", "bgnn_epoch_reset", "bgnn_training_targets"]
    assert sorted(runtime._TRAINER_SIGNATURES) == sorted(decl)
    for s, n_args in decl.items():
        assert len(runtime._TRAINER_SIGNATURES[s][1]) == n_args, s
        assert runtime._TRAINER_SIGNATURES[s][0] is C.c_int
        assert hasattr(lib, s), f"{s} declared in bgnn_trainer.h but not exported"
        assert getattr(lib, s).argtypes == runtime._TRAINER_SIGNATURES[s][1]
    others = set(runtime._SIGNATURES) | set(runtime._TRAIN_SIGNATURES) | set(runtime._LOSS_SIGNATURES) | \
        set(runtime._OPTIM_SIGNATURES) | set(runtime._NOISE_SIGNATURES) | set(runtime._SIDECAR_SIGNATURES)
    assert not set(decl) & others
    assert lib.bgnn_abi_version() == 7 == runtime.ABI_VERSION


def test_trainer_header_constants_match_the_python_side():
    """The constants the header fixes are the ones the Python side uses: the normalisation floor and cap of
    config/constants.py (as float32), the accumulator's layout, the class limit of the loss pass."""
    from bathymetric_gnn_amd import runtime
    from bathymetric_gnn_amd.config.constants import CORRECTION_NORM_CAP, CORRECTION_NORM_FLOOR
    text = _header()

    def macro(name):
        return re.search(rf"#define {name} (.+)", text).group(1).strip()
    assert np.float32(macro("BGNN_CORRECTION_NORM_FLOOR").rstrip("f")) == np.float32(CORRECTION_NORM_FLOOR)
    assert np.float32(macro("BGNN_CORRECTION_NORM_CAP").rstrip("f")) == np.float32(CORRECTION_NORM_CAP)
    assert int(macro("BGNN_EPOCH_MAX_CLASSES")) == runtime.EPOCH_MAX_CLASSES == runtime.LOSS_MAX_CLASSES
    assert [int(macro(f"BGNN_EPOCH_ACC_{k}").split()[0]) for k in ("SUMS", "NODES", "CORRECT", "STEPS", "CONFUSION")] == [0, 48, 56, 64, 72]
    assert runtime.EPOCH_ACC_BYTES == 72 + 8 * 16 * 16
    assert (int(macro("BGNN_TARGETS_SYNTHETIC").split()[0]), int(macro("BGNN_TARGETS_GROUND_TRUTH").split()[0])) == \
        (runtime.TARGETS_SYNTHETIC, runtime.TARGETS_GROUND_TRUTH)


def test_trainer_header_is_plain_c(tmp_path, lib):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    from bathymetric_gnn_amd import runtime
    src = tmp_path / "trainer_abi.c"
    src.write_text('#include <dlfcn.h>\n#include <stdio.h>\n#include "bgnn_trainer.h"\n'
                   "int main(int argc, char **argv) {\n"
                   "  void *lib = argc < 2 ? 0 : dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);\n"
                   "  if (!lib) return 1;\n"
                   + "".join(f'  if (!dlsym(lib, "{s}")) {{ fprintf(stderr, "missing {s}\\n"); return 2; }}\n' for s in _declarations())
                   + '  printf("ok %d\\n", (int)BGNN_EPOCH_ACC_BYTES);\n  return 0;\n}\n')
    exe = tmp_path / "trainer_abi"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-ldl"], check=True)
    r = subprocess.run([str(exe), os.path.join(ROOT, "bathymetric-gnn_amd", "libbgnn_hip.so")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", str(runtime.EPOCH_ACC_BYTES)]


def test_stop_rule():
    """trainer.py:698-706 on a hand-written run: strict '<' against best - min_delta, the counter reset by an improvement, the
    stop when the counter reaches patience."""
    from bathymetric_gnn_amd.training.trainer import StopRule
    rule = StopRule(patience=3, min_delta=0.25)
    run = [  # validation loss -> (improved, stop), best afterwards, counter afterwards
        (2.0, (True, False), 2.0, 0),      # anything beats inf
        (1.875, (False, False), 2.0, 1),   # better by 0.125 < min_delta: no improvement
        (1.75, (False, False), 2.0, 2),    # better by exactly min_delta: '<' is strict, no improvement
        (1.5, (True, False), 1.5, 0),      # better by 0.5: improvement, the counter starts over
        (1.5, (False, False), 1.5, 1),
        (3.0, (False, False), 1.5, 2),
        (1.26, (False, True), 1.5, 3),     # the third epoch in a row without improvement: patience reached
    ]
    for loss, want, best, counter in run:
        assert rule.update(loss) == want, loss
        assert rule.best == best and rule.counter == counter, loss
    once = StopRule(patience=1, min_delta=1e9)
    assert once.update(5.0) == (True, False) and once.update(0.0) == (False, True)


def test_training_settings_accessor():
    from bathymetric_gnn_amd.config import Config
    from bathymetric_gnn_amd.training.trainer import training_settings
    reference_defaults = dict(learning_rate=1e-3, weight_decay=1e-4, batch_size=4, epochs=100, scheduler="cosine", warmup_epochs=5,
                              patience=15, min_delta=1e-4, classification_weight=1.0, correction_weight=0.5, confidence_weight=0.2,
                              class_weights=None, augment_rotations=True, augment_flips=True, augment_noise_intensity=True)
    assert vars(training_settings({})) == reference_defaults
    assert vars(training_settings(None)) == reference_defaults
    assert vars(training_settings(Config())) == reference_defaults
    s = training_settings({"learning_rate": 3e-4, "epochs": 7, "scheduler": "plateau", "no_such_key": 1})
    assert (s.learning_rate, s.epochs, s.scheduler, s.batch_size) == (3e-4, 7, "plateau", 4)
    assert not hasattr(s, "no_such_key")
    obj = SimpleNamespace(batch_size=2, patience=1, min_delta=1e9, something_else="x")
    s = training_settings(obj)
    assert (s.batch_size, s.patience, s.min_delta, s.epochs) == (2, 1, 1e9, 100) and not hasattr(s, "something_else")
    cfg = Config()
    cfg.training = {"batch_size": 8}
    assert training_settings(cfg).batch_size == 8 and isinstance(cfg.training, dict)
    assert training_settings(SimpleNamespace(training=obj)).patience == 1


def test_ground_truth_scan():
    """A 70 x 90 label band at tile 32 / overlap 8 (stride 24): 2 x 3 full tiles on the stride grid, and -- 70 and 90 are no
    multiples of 24 -- the scan's single far-corner tile.  One stride tile is labelled below min_valid_ratio and is dropped; the
    class counts run over the labelled cells of the kept tiles, overlaps counted once per tile."""
    from bathymetric_gnn_amd.training.tile_store import plan_ground_truth_tiles
    rng = np.random.default_rng(3)
    labels = rng.choice(np.array([-1, 0, 1, 2], np.int32), size=(70, 90), p=(0.2, 0.6, 0.05, 0.15)).astype(np.int32)
    labels[0:32, 48:80] = -1
    labels[3, 50:60] = 2                       # 10 of 1024 cells labelled: below 0.1
    grid_boxes = [(0, 0, 32, 32), (0, 24, 32, 56), (0, 48, 32, 80),
                  (24, 0, 56, 32), (24, 24, 56, 56), (24, 48, 56, 80)]
    corner = (38, 58, 70, 90)
    dropped = (0, 48, 32, 80)
    want_boxes = [b for b in grid_boxes if b != dropped] + [corner]
    want_counts = {c: sum(int((labels[r0:r1, c0:c1] == c).sum()) for r0, c0, r1, c1 in want_boxes) for c in (0, 1, 2)}
    boxes, counts = plan_ground_truth_tiles(labels, tile_size=32, overlap=8, min_valid_ratio=0.1)
    assert boxes == want_boxes
    assert counts == want_counts and all(v > 0 for v in counts.values())
    ratio = (labels[0:32, 48:80] >= 0).mean()
    assert 0 < ratio < 0.1
    # every kept tile reaches the ratio; with the threshold at 0 the dropped tile is back, in scan order
    assert all((labels[r0:r1, c0:c1] >= 0).mean() >= 0.1 for r0, c0, r1, c1 in boxes)
    assert plan_ground_truth_tiles(labels, 32, 8, 0.0)[0] == grid_boxes + [corner]
    # extents that are multiples of the stride: no corner tile (trainer.py:157); a raster no larger than a tile: none at all
    assert plan_ground_truth_tiles(np.zeros((72, 96), np.int32), 32, 8, 0.1)[0] == \
        [(r, c, r + 32, c + 32) for r in (0, 24) for c in (0, 24, 48)]
    assert plan_ground_truth_tiles(np.zeros((32, 90), np.int32), 32, 8, 0.1)[0] == [(0, 0, 32, 32), (0, 24, 32, 56), (0, 48, 32, 80)]


def test_training_package_exports():
    """``training.__all__`` stays the reference's loss names; the trainer's classes are importable beside them."""
    import bathymetric_gnn_amd.training as training
    from bathymetric_gnn_amd.training.tile_store import TileStore
    from bathymetric_gnn_amd.training.trainer import EpochMetrics, StopRule, Trainer
    assert training.__all__ == ["BathymetricGNNLoss", "ClassificationLoss", "CorrectionLoss", "ConfidenceCalibrationLoss",
                                "FeaturePreservationLoss", "ShoalSafetyLoss", "compute_class_weights", "compute_correction_delta"]
    for cls in (Trainer, TileStore, EpochMetrics, StopRule):
        assert getattr(training, cls.__name__) is cls
    assert training.FusedAdamW.__name__ == "FusedAdamW"


def test_step_plan_needs_no_gpu():
    """The plan of an epoch is host arithmetic: the documented permutation cut into batches, and the documented dropout seeds."""
    from bathymetric_gnn_amd.training.trainer import Trainer, dropout_seed
    t = Trainer.__new__(Trainer)
    t.seed, t.settings = 5, SimpleNamespace(batch_size=2)
    t.train_store, t.val_store = list(range(7)), list(range(3))
    plan = t.step_plan(3)
    order = np.random.default_rng([5, 3]).permutation(7)
    assert [p.tolist() for p, _ in plan] == [order[k:k + 2].tolist() for k in range(0, 7, 2)]
    assert [s for _, s in plan] == [(5 << 32) | (3 * 4 + k) for k in range(4)] == [dropout_seed(5, 12 + k) for k in range(4)]
    assert [p.tolist() for p, _ in t.step_plan(3, validation=True)] == [[0, 1], [2]]
    assert all(s is None for _, s in t.step_plan(3, validation=True))
    assert [p.tolist() for p, _ in t.step_plan(4)] != [p.tolist() for p, _ in plan]
