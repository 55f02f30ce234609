"""Synthetic noise generation -- drop-in for the reference's ``data/synthetic_noise.py``, computed on the GPU.

``SyntheticNoiseGenerator``, ``NoiseAugmentor`` and ``NoiseLabel`` keep the reference's constructor arguments, defaults and
attribute names (``data/synthetic_noise.py:25-33, 43-96, 418-434``).  ``generate`` takes host arrays like the reference's;
``generate_batch`` takes clean tiles that already live in HBM (the flat layout of ``GraphBuilder.build_from_device``) and
returns flat device tensors, and ``training_targets`` turns them into the per-node labels of
``BathymetricGraphDataset.__getitem__`` (``training/trainer.py:400-424``) without leaving the device.

Every formula is the reference's (include/bgnn_noise.h lists them).  What differs is WHICH cells the random fields pick:
numpy's stream cannot be followed on the device, so the per-cell draws come from the documented counter-based generator keyed
on (seed, sample index, stream, cell), and the scalar draws of sample ``i`` from ``numpy.random.default_rng([seed, i])`` -- the
same (seed, sample index) gives the same sample bit for bit, whatever batch it is generated in.  Every draw can be supplied
instead (``draws=``).
"""
from __future__ import annotations

import ctypes as C
import logging
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import runtime as rt
from ..config.constants import CORRECTION_NORM_CAP, CORRECTION_NORM_FLOOR

logger = logging.getLogger(__name__)

FIELD_DTYPES = {"gaussian": torch.float64, "uniform": torch.float64, "sign": torch.int8, "magnitude": torch.float64}


@dataclass
class NoiseLabel:
    """Labels for synthetic noise generation."""
    noisy_depth: np.ndarray           # Depth with noise added
    clean_depth: np.ndarray           # Original clean depth
    noise_mask: np.ndarray            # Boolean mask where noise was added
    noise_magnitude: np.ndarray       # Magnitude of noise at each point
    classification: np.ndarray        # Per-pixel class (0=seafloor, 2=noise) - model convention


@dataclass
class NoiseBatch:
    """What ``generate_batch`` returns: flat device tensors in the layout of the input tiles, and the plans that made them."""
    hw: np.ndarray                    # int32 [T, 2]
    noisy_depth: torch.Tensor         # float32 [cells]
    noise_mask: torch.Tensor          # bool [cells]
    noise_magnitude: torch.Tensor     # float32 [cells]
    classification: torch.Tensor      # int64 [cells]
    plans: List[Dict[str, Any]]       # the scalar draws of every tile
    sample_indices: List[int]


class SyntheticNoiseGenerator:
    """Generates realistic synthetic noise for bathymetric data (reference class of the same name), on the GPU."""

    def __init__(
        self,
        enable_gaussian: bool = True,
        gaussian_std_range: Tuple[float, float] = (0.1, 0.5),
        enable_spikes: bool = True,
        spike_magnitude_range: Tuple[float, float] = (1.0, 5.0),
        spike_density_range: Tuple[float, float] = (0.001, 0.01),
        enable_blobs: bool = True,
        blob_size_range: Tuple[int, int] = (3, 15),
        blob_count_range: Tuple[int, int] = (5, 50),
        blob_magnitude_range: Tuple[float, float] = (0.5, 3.0),
        enable_systematic: bool = True,
        systematic_amplitude_range: Tuple[float, float] = (0.2, 1.0),
        complexity_correlation: float = 0.3,
        seed: Optional[int] = None,
    ):
        rt.load_library()
        self.enable_gaussian = enable_gaussian
        self.gaussian_std_range = gaussian_std_range
        self.enable_spikes = enable_spikes
        self.spike_magnitude_range = spike_magnitude_range
        self.spike_density_range = spike_density_range
        self.enable_blobs = enable_blobs
        self.blob_size_range = blob_size_range
        self.blob_count_range = blob_count_range
        self.blob_magnitude_range = blob_magnitude_range
        self.enable_systematic = enable_systematic
        self.systematic_amplitude_range = systematic_amplitude_range
        self.complexity_correlation = complexity_correlation
        self.rng = np.random.default_rng(seed)
        # the key of every draw; an unseeded generator takes one from its numpy Generator
        self.seed = int(seed) if seed is not None else int(self.rng.integers(0, 2 ** 63))
        self.next_sample = 0              # sample index the next generate / generate_batch starts from
        self.device = None                # None: the current GPU

    # ---- scalar draws --------------------------------------------------------------------------
    def draw_plan(self, sample: int, intensity: float = 1.0, given: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
        """The scalar draws of sample ``sample`` in the reference's order, from ``default_rng([seed, sample])``; entries of
        ``given`` replace the drawn ones.  Blob centres are a uniform draw ``u``: the device takes the floor(u * n_valid)-th
        valid cell."""
        rng = np.random.default_rng([self.seed & (2 ** 64 - 1), int(sample)])
        intensity = float(intensity)
        p: Dict[str, Any] = {"sample": int(sample), "intensity": intensity, "gaussian_std_factor": 0.0, "spike_density_draw": 0.0,
                             "blobs": [], "artifact": "none", "amplitude_factor": 0.0, "freq_a": 0.0, "freq_b": 0.0, "phase": 0.0}
        if self.enable_gaussian:
            p["gaussian_std_factor"] = float(rng.uniform(*self.gaussian_std_range))
        if self.enable_spikes:
            p["spike_density_draw"] = float(rng.uniform(*self.spike_density_range))
        if self.enable_blobs:
            lo, hi = self.blob_count_range
            n = int(rng.integers(int(lo * intensity), int(hi * intensity) + 1))
            for _ in range(n):
                u = float(rng.random())
                size = int(rng.integers(self.blob_size_range[0], self.blob_size_range[1] + 1))
                m = float(rng.uniform(*self.blob_magnitude_range))
                if rng.random() < 0.2:          # occasionally negative (shadows)
                    m = -m
                p["blobs"].append((-1, u, size, m))
        if self.enable_systematic:
            kind = ("stripe", "wave", "gradient")[int(rng.integers(3))]
            p["amplitude_factor"] = float(rng.uniform(*self.systematic_amplitude_range))
            if kind == "stripe":
                p["artifact"] = ("stripe_horizontal", "stripe_vertical")[int(rng.integers(2))]
                p["freq_a"] = float(rng.uniform(0.01, 0.05))
            elif kind == "wave":
                p["artifact"] = "wave"
                p["freq_a"], p["freq_b"] = float(rng.uniform(0.005, 0.02)), float(rng.uniform(0.005, 0.02))
                p["phase"] = float(rng.uniform(0, 2 * np.pi))
            else:
                p["artifact"] = ("gradient_x", "gradient_y", "gradient_diagonal")[int(rng.integers(3))]
        for k, v in (given or {}).items():
            if k in p and k not in ("sample", "intensity"):
                p[k] = v
        if not isinstance(p["artifact"], str):
            p["artifact"] = rt.NOISE_ARTIFACTS[int(p["artifact"])]
        if p["artifact"] not in rt.NOISE_ARTIFACTS:
            raise ValueError(f"unknown artifact {p['artifact']!r}")
        return p

    def _params(self) -> rt.NoiseParams:
        return rt.NoiseParams(int(bool(self.enable_gaussian)), int(bool(self.enable_spikes)), int(bool(self.enable_blobs)),
                              int(bool(self.enable_systematic)), float(self.complexity_correlation),
                              float(self.spike_magnitude_range[0]), float(self.spike_magnitude_range[1]),
                              self.seed & (2 ** 64 - 1))

    # ---- device batch ---------------------------------------------------------------------------
    def generate_batch(self, hw: np.ndarray, depth_t: torch.Tensor, mask_t: Optional[torch.Tensor] = None,
                       intensities: Optional[Sequence[float]] = None, draws: Optional[Sequence[Optional[Dict[str, Any]]]] = None,
                       sample_indices: Optional[Sequence[int]] = None, ctx: Optional[rt.Context] = None) -> NoiseBatch:
        """Noise for a batch of clean tiles on the device.  ``hw`` int32 [T, 2]; ``depth_t`` float32 [cells] and ``mask_t``
        uint8 / bool [cells] (None: ``isfinite(depth)``) flat, concatenated row-major, as ``GraphBuilder.build_from_device``
        takes them.  ``intensities``: one per tile (default 1.0).  ``sample_indices``: the sample index of every tile (default:
        the generator's running count).  ``draws``: per tile a dict of supplied draws -- the scalars of ``draw_plan``
        (``gaussian_std_factor``, ``spike_density_draw``, ``blobs`` [(row, col, size, signed magnitude draw)], ``artifact``,
        ``amplitude_factor``, ``freq_a``, ``freq_b``, ``phase``) and the per-cell fields ``gaussian`` (the final noise field,
        float64), ``uniform`` (float64), ``sign`` (int8) and ``magnitude`` (float64) as [h, w] arrays or tensors; a field is
        supplied for every tile of the batch or for none."""
        ctx = ctx if ctx is not None else rt.get_context(self.device)
        hw = np.ascontiguousarray(hw, np.int32).reshape(-1, 2)
        T = hw.shape[0]
        cells = int((hw[:, 0].astype(np.int64) * hw[:, 1]).sum())
        if depth_t.dtype != torch.float32 or depth_t.numel() != cells or not depth_t.is_cuda:
            raise ValueError("depth_t must be a float32 device tensor with one entry per cell of the tile table")
        depth_t = depth_t.contiguous().view(-1)
        if mask_t is None:
            mask_t = torch.isfinite(depth_t)
        if mask_t.numel() != cells or mask_t.dtype not in (torch.uint8, torch.bool):
            raise ValueError("mask_t must be a uint8 / bool device tensor with one entry per cell")
        mask_t = mask_t.contiguous().view(-1)
        if sample_indices is None:
            sample_indices = list(range(self.next_sample, self.next_sample + T))
            self.next_sample += T
        intensities = [1.0] * T if intensities is None else [float(v) for v in intensities]
        draws = [None] * T if draws is None else list(draws)
        if not (len(sample_indices) == len(intensities) == len(draws) == T):
            raise ValueError("intensities, draws and sample_indices need one entry per tile")
        plans = [self.draw_plan(s, i, d) for s, i, d in zip(sample_indices, intensities, draws)]

        c_plans = (rt.NoisePlan * T)()
        blobs: List[rt.NoiseBlob] = []
        for t, p in enumerate(plans):
            first = len(blobs)
            for row, col, size, m in p["blobs"]:
                if row < 0:
                    blobs.append(rt.NoiseBlob(-1, -1, int(size), 0, float(col), float(m)))
                else:
                    blobs.append(rt.NoiseBlob(int(row), int(col), int(size), 0, 0.0, float(m)))
            c_plans[t] = rt.NoisePlan(int(p["sample"]) & (2 ** 64 - 1), p["intensity"], float(p["gaussian_std_factor"]),
                                      float(p["spike_density_draw"]) * p["intensity"], float(p["amplitude_factor"]),
                                      float(p["freq_a"]), float(p["freq_b"]), float(p["phase"]),
                                      rt.NOISE_ARTIFACTS.index(p["artifact"]), first, len(blobs) - first, 0)
        c_blobs = (rt.NoiseBlob * max(len(blobs), 1))(*blobs)

        dev = ctx.device
        fields = rt.NoiseFields()
        keep = []
        for name, dt in FIELD_DTYPES.items():
            have = [d is not None and name in d for d in draws]
            if not any(have):
                continue
            if not all(have):
                raise ValueError(f"the per-cell draw {name!r} is supplied for some tiles of the batch only")
            parts = [torch.as_tensor(d[name]).to(device=dev, dtype=dt).reshape(-1) for d in draws]
            if any(p.numel() != int(hw[t, 0]) * int(hw[t, 1]) for t, p in enumerate(parts)):
                raise ValueError(f"the per-cell draw {name!r} does not have the shape of its tile")
            f = torch.cat(parts) if T > 1 else parts[0].contiguous()
            keep.append(f)
            setattr(fields, name, f.data_ptr())

        lib = ctx.lib
        hw_p = hw.ctypes.data_as(C.c_void_p)
        ws_bytes = lib.bgnn_noise_workspace_bytes(T, hw_p, len(blobs))
        ws = torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8, device=dev)
        noisy = torch.empty(cells, dtype=torch.float32, device=dev)
        nmask = torch.empty(cells, dtype=torch.uint8, device=dev)
        mag = torch.empty(cells, dtype=torch.float32, device=dev)
        cls = torch.empty(cells, dtype=torch.int64, device=dev)
        params = self._params()
        ctx.begin()
        rt.check(lib.bgnn_noise_generate(ctx.handle, T, hw_p, rt.ptr(depth_t), rt.ptr(mask_t), C.byref(params), c_plans, c_blobs,
                                         len(blobs), C.byref(fields), rt.ptr(ws), int(ws_bytes), rt.ptr(noisy), rt.ptr(nmask),
                                         rt.ptr(mag), rt.ptr(cls)))
        ctx.end()
        # the workspace and the supplied fields are read by work queued on the library's stream
        for t_ in [ws, depth_t, mask_t] + keep:
            t_.record_stream(ctx.stream)
        return NoiseBatch(hw, noisy, nmask.view(torch.bool), mag, cls, plans, [int(s) for s in sample_indices])

    # ---- reference API ----------------------------------------------------------------------------
    def generate(self, clean_depth: np.ndarray, valid_mask: Optional[np.ndarray] = None, intensity: float = 1.0) -> NoiseLabel:
        """Add synthetic noise to clean bathymetric data (reference ``generate``, :98-181): host arrays in, a ``NoiseLabel``
        of numpy arrays out (float32 depth and magnitude, bool mask, int64 classification)."""
        ctx = rt.get_context(self.device)
        d = np.asarray(clean_depth)
        if d.ndim != 2:
            raise ValueError(f"clean_depth must be a 2-D grid, got shape {d.shape}")
        d32 = np.ascontiguousarray(d, np.float32)
        m = np.isfinite(d32) if valid_mask is None else np.asarray(valid_mask, dtype=bool)
        if m.shape != d32.shape:
            raise ValueError(f"valid_mask shape {m.shape} != depth shape {d32.shape}")
        hw = np.array([d32.shape], np.int32)
        depth_t = torch.from_numpy(d32.ravel()).to(ctx.device)
        mask_t = torch.from_numpy(np.ascontiguousarray(m).ravel().view(np.uint8)).to(ctx.device)
        b = self.generate_batch(hw, depth_t, mask_t, [intensity])
        shape = d32.shape
        label = NoiseLabel(noisy_depth=b.noisy_depth.cpu().numpy().reshape(shape), clean_depth=clean_depth,
                           noise_mask=b.noise_mask.cpu().numpy().reshape(shape),
                           noise_magnitude=b.noise_magnitude.cpu().numpy().reshape(shape),
                           classification=b.classification.cpu().numpy().reshape(shape))
        logger.debug("Generated noise: %d noisy cells", int(label.noise_mask.sum()))
        return label


class NoiseAugmentor:
    """Applies noise augmentation during training (reference class of the same name): a random intensity per sample, drawn
    from ``default_rng([seed, sample index])``."""

    def __init__(
        self,
        base_generator: SyntheticNoiseGenerator,
        intensity_range: Tuple[float, float] = (0.5, 1.5),
        seed: Optional[int] = None,
    ):
        self.generator = base_generator
        self.intensity_range = intensity_range
        self.rng = np.random.default_rng(seed)
        self.seed = int(seed) if seed is not None else int(self.rng.integers(0, 2 ** 63))

    def intensity(self, sample: int) -> float:
        return float(np.random.default_rng([self.seed & (2 ** 64 - 1), int(sample)]).uniform(*self.intensity_range))

    def __call__(self, clean_depth: np.ndarray, valid_mask: Optional[np.ndarray] = None) -> NoiseLabel:
        """Generate augmented noisy sample."""
        return self.generator.generate(clean_depth, valid_mask, self.intensity(self.generator.next_sample))

    def augment_batch(self, hw: np.ndarray, depth_t: torch.Tensor, mask_t: Optional[torch.Tensor] = None,
                      sample_indices: Optional[Sequence[int]] = None, ctx: Optional[rt.Context] = None) -> NoiseBatch:
        """``generate_batch`` with a drawn intensity per tile."""
        T = int(np.asarray(hw).reshape(-1, 2).shape[0])
        if sample_indices is None:
            sample_indices = list(range(self.generator.next_sample, self.generator.next_sample + T))
            self.generator.next_sample += T
        return self.generator.generate_batch(hw, depth_t, mask_t, [self.intensity(s) for s in sample_indices],
                                             sample_indices=sample_indices, ctx=ctx)


def training_targets(graph, clean_t: torch.Tensor, noisy_t: torch.Tensor, classification_t: torch.Tensor,
                     noise_mask_t: torch.Tensor):
    """The labels ``BathymetricGraphDataset.__getitem__`` attaches to a graph (``training/trainer.py:400-424``), per node and on
    the device: ``y`` (int64), ``correction_target`` = clamp((noisy - clean) / clamp(local_std, min=CORRECTION_NORM_FLOOR),
    +-CORRECTION_NORM_CAP) and ``noise_mask`` (bool), gathered at the graph's ``valid_rows`` / ``valid_cols``.  ``graph``: what
    ``GraphBuilder.build_from_device`` returned for ``noisy_t``; the four tensors are flat, in the layout of that batch."""
    hw = np.asarray(graph._hw, np.int64)
    dev = graph.device
    off = torch.as_tensor(np.concatenate([[0], np.cumsum(hw[:, 0] * hw[:, 1])[:-1]]), device=dev)
    width = torch.as_tensor(hw[:, 1].copy(), device=dev)
    b = graph.batch
    idx = off[b] + graph.valid_rows * width[b] + graph.valid_cols
    y = classification_t.view(-1)[idx].long()
    raw = noisy_t.view(-1)[idx] - clean_t.view(-1)[idx]
    norm_scale = torch.clamp(graph.local_std, min=CORRECTION_NORM_FLOOR)
    target = torch.clamp(raw.float() / norm_scale, min=-CORRECTION_NORM_CAP, max=CORRECTION_NORM_CAP)
    return y, target, noise_mask_t.view(-1)[idx].bool()
