#!/usr/bin/env python3
"""Golden vectors for the synthetic-noise generator, produced by the REFERENCE's own ``data/synthetic_noise.py``:

    python tests/golden/make_golden_noise.py /path/to/reference

The module is loaded by file path (the reference's ``data/__init__`` pulls in GDAL / PyG modules).  ``generator.rng`` is replaced
by a wrapper that records every draw; the records become the injected draws of a fixture (``noise/<case>.npz``), the spike
lists scattered to the cells the reference picked.  Each fixture holds the clean tile, the draws, the reference's four outputs
on the float32 tile (ref32), its ``noisy_depth`` on the float64 copy of the tile with the same seed (ref64), and ``np.std`` of
the valid depths in both precisions.  ``noise/signatures.json`` holds the constructor names and defaults.

The asserts look at the reference's outputs; the near-threshold count uses the float64 restatement of tests/_noise_cpu.py.
"""
import importlib.util
import inspect
import json
import os
import sys

sys.dont_write_bytecode = True
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _noise_cpu as nc  # noqa: E402
from _conditioning import BOUND_C  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BGNN_REFERENCE", "")
spec = importlib.util.spec_from_file_location("ref_synthetic_noise", os.path.join(REF, "data", "synthetic_noise.py"))
sn = importlib.util.module_from_spec(spec)
sys.modules["ref_synthetic_noise"] = sn
spec.loader.exec_module(sn)
OUT = os.path.join(HERE, "noise")


class Recorder:
    """Stands in for a numpy Generator: forwards every call and keeps (name, result)."""

    def __init__(self, rng):
        self._rng, self.log = rng, []

    def __getattr__(self, name):
        fn = getattr(self._rng, name)

        def call(*a, **k):
            r = fn(*a, **k)
            self.log.append((name, r))
            return r
        return call


class Gen(sn.SyntheticNoiseGenerator):
    def _add_spike_noise(self, depth, valid_mask, noise_mask, noise_magnitude, depth_range, complexity, intensity):
        self.seen_complexity = complexity.copy()
        return super()._add_spike_noise(depth, valid_mask, noise_mask, noise_magnitude, depth_range, complexity, intensity)


def clean_tile(h, w, seed, kind="field"):
    rng = np.random.default_rng(1000 + seed)
    r, c = np.mgrid[:h, :w].astype(np.float64)
    d = -30 + 1.5 * np.sin(r / 9.0 + rng.uniform(0, 6)) * np.cos(c / 7.0) + 0.04 * c + 0.8 * np.exp(-((r - h / 3) ** 2 + (c - w / 2) ** 2) / 40.0)
    d += 0.05 * rng.standard_normal((h, w))
    if kind == "constant":
        d[:] = -25.5
    return d.astype(np.float32)


def run(depth, mask_arg, intensity, seed, **kw):
    g = Gen(seed=seed, **kw)
    g.rng = Recorder(g.rng)
    out = g.generate(depth, mask_arg, intensity)
    return g, out


def parse(g, valid, intensity):
    """The recorded draws in the order generate() makes them."""
    log, p = g.rng.log, 0

    def take(name):
        nonlocal p
        assert log[p][0] == name, (p, log[p][0], name)
        p += 1
        return log[p - 1][1]
    h, w = valid.shape
    d = {"scalars": np.zeros(7), "blobs": np.zeros((0, 4)), "gaussian_field": np.zeros((h, w)), "uniform_field": np.ones((h, w)),
         "spike_index": np.zeros(0, np.int32), "spike_sign": np.zeros(0, np.int8), "spike_magnitude": np.zeros(0)}
    if not valid.any():
        assert not log
        return d
    if g.enable_gaussian:
        d["scalars"][0] = take("uniform")
        d["gaussian_field"] = take("normal")
    if g.enable_spikes:
        d["scalars"][1] = take("uniform")
        d["uniform_field"] = take("random")
        loc = (d["uniform_field"] < d["scalars"][1] * intensity * (1 + g.complexity_correlation * (g.seen_complexity - 0.5))) & valid
        if loc.any():
            signs, mags = take("choice"), take("uniform")
            assert len(signs) == len(mags) == int(loc.sum()), "spike count differs from the recorded choice draw"
            d["spike_index"] = np.flatnonzero(loc.ravel()).astype(np.int32)
            d["spike_sign"], d["spike_magnitude"] = signs.astype(np.int8), mags
    if g.enable_blobs:
        n = int(take("integers"))
        cells = np.argwhere(valid)
        blobs = []
        for _ in range(n):
            r, c = cells[int(take("integers"))]
            size, m = int(take("integers")), float(take("uniform"))
            blobs.append((r, c, size, -m if take("random") < 0.2 else m))
        d["blobs"] = np.array(blobs, np.float64).reshape(-1, 4)
    if g.enable_systematic:
        kind = str(take("choice"))
        d["scalars"][3] = take("uniform")
        if kind == "stripe":
            o = str(take("choice"))
            d["scalars"][2] = 1 if o == "horizontal" else 2
            d["scalars"][4] = take("uniform")
        elif kind == "wave":
            d["scalars"][2] = 3
            d["scalars"][4], d["scalars"][5], d["scalars"][6] = take("uniform"), take("uniform"), take("uniform")
        else:
            d["scalars"][2] = {"x": 4, "y": 5, "diagonal": 6}[str(take("choice"))]
    assert p == len(log), "unparsed draws"
    return d


def make(name, h, w, seed, intensity=1.0, holes=0.0, nan_holes=False, kind="field", none_valid=False, **kw):
    depth = clean_tile(h, w, seed, kind)
    hole = np.random.default_rng(2000 + seed).random((h, w)) < holes
    if none_valid:
        hole[:] = True
    depth[hole] = np.float32(np.nan) if nan_holes else np.float32(1.0e6)
    valid = ~hole
    mask_arg = None if nan_holes else valid
    g, o32 = run(depth, mask_arg, intensity, seed, **kw)
    d = parse(g, valid, intensity)
    _, o64 = run(depth.astype(np.float64), mask_arg, intensity, seed, **kw)
    assert o32.noisy_depth.dtype == np.float32 and o64.noisy_depth.dtype == np.float64
    assert np.array_equal(o32.noise_mask, o64.noise_mask), f"{name}: ref32 and ref64 mark different cells"
    vd = depth[valid]
    std32, std64 = (np.std(vd), np.std(vd.astype(np.float64))) if valid.any() else (np.float32(0), 0.0)
    fx = dict(clean_depth=depth, valid_mask=valid, mask_none=np.bool_(nan_holes), intensity=np.float64(intensity),
              enable=np.array([g.enable_gaussian, g.enable_spikes, g.enable_blobs, g.enable_systematic], np.int8),
              complexity_correlation=np.float64(g.complexity_correlation), spike_magnitude_range=np.array(g.spike_magnitude_range, np.float64),
              noisy_depth=o32.noisy_depth, noise_mask=o32.noise_mask, noise_magnitude=o32.noise_magnitude,
              classification=o32.classification, noisy_depth64=o64.noisy_depth, std32=np.float32(std32), std64=np.float64(std64), **d)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **fx)
    assert os.path.getsize(path) <= 600_000, (name, os.path.getsize(path))
    # near-threshold cells, by the float64 restatement driven with these draws
    dep, val, plan, params, fields, _ = nc.load_fixture(path)
    _, _, _, _, info = nc.generate(dep, val, plan, params, fields=fields)
    if valid.any() and kind != "constant":      # (a constant tile has every term zero: it is compared exactly, without exceptions)
        bound = BOUND_C * float(np.abs(o32.noisy_depth.astype(np.float64) - o64.noisy_depth)[valid].max())
        near = int(nc.near_threshold(info, valid, bound).sum())
        assert near <= 0.001 * valid.sum(), (name, near, int(valid.sum()))
    print(f"{name}: {h}x{w} artifact={nc.ARTIFACTS[int(d['scalars'][2])]} spikes={len(d['spike_index'])} blobs={len(d['blobs'])} "
          f"marked={int(o32.noise_mask.sum())} bytes={os.path.getsize(path)}")
    return int(d["scalars"][2])


def main():
    os.makedirs(OUT, exist_ok=True)
    kinds = {}                                                           # every systematic variant: the first seed that draws it
    for seed in range(200):
        depth = clean_tile(64, 48, seed)
        valid = np.ones(depth.shape, bool)
        kind = int(parse(run(depth, valid, 1.0, seed)[0], valid, 1.0)["scalars"][2])
        if kind not in kinds:
            kinds[kind] = seed
            assert make(f"all_{nc.ARTIFACTS[kind]}", 64, 48, seed) == kind
        if len(kinds) == 6:
            break
    assert sorted(kinds) == [1, 2, 3, 4, 5, 6], kinds
    off = dict(enable_gaussian=False, enable_spikes=False, enable_blobs=False, enable_systematic=False)
    for k in off:
        make("only_" + k[7:], 48, 40, 2, **{**off, k: True})
    make("intensity_050", 48, 40, 3, intensity=0.5)
    make("intensity_150", 48, 40, 5, intensity=1.5)
    make("holes10", 64, 48, 7, holes=0.10)
    make("nan_mask_none", 40, 56, 9, holes=0.08, nan_holes=True)
    make("constant", 32, 40, 10, kind="constant")
    make("no_valid", 16, 24, 11, none_valid=True)
    sig = {}
    for cls in (sn.SyntheticNoiseGenerator, sn.NoiseAugmentor):
        sig[cls.__name__] = [[n, None if p.default is inspect.Parameter.empty else p.default]
                             for n, p in inspect.signature(cls.__init__).parameters.items() if n != "self"]
    sig["generate"] = [[n, None if p.default is inspect.Parameter.empty else p.default]
                       for n, p in inspect.signature(sn.SyntheticNoiseGenerator.generate).parameters.items() if n != "self"]
    sig["NoiseLabel"] = [f.name for f in sn.NoiseLabel.__dataclass_fields__.values()]
    json.dump(sig, open(os.path.join(OUT, "signatures.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
