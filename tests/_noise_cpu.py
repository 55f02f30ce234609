"""numpy restatement of csrc/synthetic_noise.hip and of the counter-based generator of include/bgnn_noise.h.

``generate`` walks one tile through the four noise terms of the reference's ``SyntheticNoiseGenerator.generate`` with the
arithmetic the kernels use: per-tile scalars accumulated in float64 and rounded where numpy holds a float32, the windowed
standard deviation in float64 stored as float32, the reference's float32 / float64 mix in every term.  It takes the same plan
(scalars + blob list) and the same optional injected per-cell fields as ``bgnn_noise_generate``.  tests/test_host_noise.py pins
it against the reference's recorded outputs; tests/test_gpu_noise.py then uses it as the yardstick for the device's own draws.
"""
import numpy as np

GOLD = 0x9E3779B97F4A7C15
STEP = 0xD1B54A32D192ED03
M64 = (1 << 64) - 1
STREAM_NORMAL_A, STREAM_NORMAL_B, STREAM_SPIKE_U, STREAM_SPIKE_SIGN, STREAM_SPIKE_MAG = 1, 2, 3, 4, 5
ARTIFACTS = ("none", "stripe_horizontal", "stripe_vertical", "wave", "gradient_x", "gradient_y", "gradient_diagonal")


def _fin(z):
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sample_key(seed, sample):
    return int(_fin(np.uint64((int(seed) + GOLD * (int(sample) + 1)) & M64)))


def bits(seed, sample, stream, index):
    """64 random bits per entry of ``index`` (uint64 array): fin(key + GOLD (stream + 1) + STEP index), key = sample_key."""
    with np.errstate(over="ignore"):
        base = np.uint64((sample_key(seed, sample) + GOLD * (int(stream) + 1)) & M64)
        return _fin(base + np.uint64(STEP) * np.asarray(index, np.uint64))


def uniform(seed, sample, stream, index):
    """53-bit uniform in [0, 1)."""
    return (bits(seed, sample, stream, index) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def normal(seed, sample, index):
    """Box-Muller in float64: sqrt(-2 ln u1) cos(2 pi u2), u1 in (0, 1] from stream 1, u2 in [0, 1) from stream 2."""
    u1 = ((bits(seed, sample, STREAM_NORMAL_A, index) >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53
    u2 = uniform(seed, sample, STREAM_NORMAL_B, index)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos((2.0 * np.pi) * u2)


def sign(seed, sample, index):
    """+1 where bit 63 of stream 4 is set, else -1."""
    return np.where(bits(seed, sample, STREAM_SPIKE_SIGN, index) >> np.uint64(63), 1, -1).astype(np.int8)


def local_std(filled):
    """Population std over the 11 x 11 window, edge mode nearest, float64 two-pass, stored float32."""
    h, w = filled.shape
    p = np.pad(filled.astype(np.float64), 5, mode="edge")
    win = np.lib.stride_tricks.sliding_window_view(p, (11, 11)).reshape(h, w, 121)
    mean = win.sum(-1) / 121.0
    return np.sqrt(((win - mean[..., None]) ** 2).sum(-1) / 121.0).astype(np.float32)


def linspace_pm1(n):
    """np.linspace(-1, 1, n) element by element."""
    i = np.arange(n, dtype=np.float64)
    if n == 1:
        return i * 2.0 + -1.0
    y = i * (2.0 / (n - 1)) + -1.0
    y[-1] = 1.0
    return y


def kth_valid_cell(valid, u):
    """Blob centre: the floor(u * n_valid)-th valid cell in row-major order."""
    idx = np.flatnonzero(valid.ravel())
    k = min(int(u * len(idx)), len(idx) - 1)
    return divmod(int(idx[k]), valid.shape[1])


def _scale32(factor, base32, intensity):
    """python float * np.float32 * python float under numpy 2: both python floats are weak, the products are float32."""
    return np.float32(np.float32(np.float32(factor) * base32) * np.float32(intensity))


def generate(depth, valid, plan, params, seed=0, fields=None):
    """One tile.  ``depth`` float32 [h, w], ``valid`` bool.  ``params``: enable_gaussian / enable_spikes / enable_blobs /
    enable_systematic, complexity_correlation, spike_magnitude_range.  ``plan``: sample, intensity, gaussian_std_factor,
    spike_density (draw x intensity), blobs [(row, col, size, signed magnitude factor)] -- row < 0: col holds the centre draw u
    --, artifact (index into ARTIFACTS), amplitude_factor, freq_a, freq_b, phase.  ``fields``: injected per-cell draws
    (gaussian f64, uniform f64, sign i8, magnitude f64), any may be missing.  Returns noisy, noise_mask, magnitude,
    classification, and a dict of intermediates (scalars, density map, float64 compared quantities) for threshold checks."""
    fields = fields or {}
    depth = np.ascontiguousarray(depth, np.float32)
    valid = np.asarray(valid, bool)
    h, w = depth.shape
    noisy = depth.copy()
    mask = np.zeros((h, w), bool)
    mag = np.zeros((h, w), np.float32)
    info = {}
    cell = np.arange(h * w, dtype=np.uint64).reshape(h, w)
    sample, inten = int(plan["sample"]), float(plan["intensity"])
    nv = int(valid.sum())
    if nv == 0:
        return noisy, mask, mag, np.zeros((h, w), np.int64), info
    # per-tile scalars: float64 accumulation, rounded where numpy holds a float32
    nn = ~np.isnan(depth)
    with np.errstate(invalid="ignore", divide="ignore"):
        nanmean = np.float32(depth[nn].astype(np.float64).sum() / nn.sum())
    vd = depth[valid].astype(np.float64)
    mean = vd.sum() / nv
    std32 = np.float32(np.sqrt(((vd - mean) ** 2).sum() / nv))
    range32 = np.float32(depth[valid].max()) - np.float32(depth[valid].min())
    ls = local_std(np.where(valid, depth, nanmean))
    lmin, lmax = ls.min(), ls.max()
    cx = (ls - lmin) / (lmax - lmin) if lmax > lmin else np.zeros_like(ls)
    info.update(nanmean=nanmean, depth_std=std32, depth_range=range32, local_std=ls, complexity=cx)

    if params["enable_gaussian"]:
        ns = _scale32(plan["gaussian_std_factor"], std32, inten)
        g64 = fields["gaussian"] if "gaussian" in fields else 0.0 + np.float64(ns) * normal(seed, sample, cell)
        g32 = np.asarray(g64, np.float64).astype(np.float32)
        noisy[valid] += g32[valid]
        mask |= valid & (np.abs(g32) > np.float32(2) * ns)
        mag[valid] = np.maximum(mag[valid], np.abs(g32[valid]))
        info.update(noise_std=ns, gaussian64=np.asarray(g64, np.float64))

    if params["enable_spikes"]:
        dens = np.float32(plan["spike_density"]) * (np.float32(1) + np.float32(params["complexity_correlation"]) * (cx - np.float32(0.5)))
        u = fields["uniform"] if "uniform" in fields else uniform(seed, sample, STREAM_SPIKE_U, cell)
        loc = (u < dens.astype(np.float64)) & valid
        sg = fields["sign"] if "sign" in fields else sign(seed, sample, cell)
        lo, hi = (float(v) for v in params["spike_magnitude_range"])
        md = fields["magnitude"] if "magnitude" in fields else lo + (hi - lo) * uniform(seed, sample, STREAM_SPIKE_MAG, cell)
        val = sg.astype(np.float64) * ((np.asarray(md, np.float64) * np.float64(range32)) * inten)
        noisy[loc] = (noisy[loc].astype(np.float64) + val[loc]).astype(np.float32)
        mask |= loc
        mag[loc] = np.abs(val[loc]).astype(np.float32)
        info.update(density=dens, spike_u=np.asarray(u, np.float64), spikes=loc)

    blob_cells = np.zeros((h, w), bool)
    centres = []
    if params["enable_blobs"]:
        rr, cc = np.ogrid[:h, :w]
        for row, col, size, factor in plan["blobs"]:
            if row < 0:
                row, col = kth_valid_cell(valid, float(col))
            row, col, size = int(row), int(col), int(size)
            centres.append((row, col))
            d2 = (rr - row) ** 2 + (cc - col) ** 2
            dist = np.sqrt(d2.astype(np.float64))
            area = (d2 < size * size) & valid
            m32 = _scale32(factor, range32, inten)
            c = np.exp(-(dist * dist) / (2.0 * (size / 2.0) ** 2)) * np.float64(m32)
            noisy[area] = (noisy[area].astype(np.float64) + c[area]).astype(np.float32)
            mask |= area
            blob_cells |= area
            mag[area] = np.maximum(mag[area], np.abs(c[area]).astype(np.float32))
    info.update(blob_cells=blob_cells, blob_centres=centres)

    kind = ARTIFACTS[int(plan["artifact"])] if params["enable_systematic"] else "none"
    if kind != "none":
        amp = _scale32(plan["amplitude_factor"], std32, inten)
        a64 = np.float64(amp)
        rows = np.arange(h, dtype=np.float64)[:, None] * np.ones((1, w))
        cols = np.ones((h, 1)) * np.arange(w, dtype=np.float64)[None, :]
        fa, fb, ph = float(plan["freq_a"]), float(plan["freq_b"]), float(plan["phase"])
        if kind == "stripe_horizontal":
            art = a64 * np.sin(((2 * np.pi) * fa) * rows)
        elif kind == "stripe_vertical":
            art = a64 * np.sin(((2 * np.pi) * fa) * cols)
        elif kind == "wave":
            art = a64 * np.sin((2 * np.pi) * (fa * cols + fb * rows) + ph)
        elif kind == "gradient_x":
            art = (a64 * linspace_pm1(w))[None, :] * np.ones((h, 1))
        elif kind == "gradient_y":
            art = (a64 * linspace_pm1(h))[:, None] * np.ones((1, w))
        else:
            art = a64 * (linspace_pm1(w)[None, :] + linspace_pm1(h)[:, None]) / 2
        a32 = art.astype(np.float32)
        noisy[valid] += a32[valid]
        mask |= valid & (np.abs(a32) > amp * np.float32(0.5))
        mag[valid] = np.maximum(mag[valid], np.abs(a32[valid]))
        info.update(amplitude=amp, artifact64=art)
    return noisy, mask, mag, np.where(mask, 2, 0).astype(np.int64), info


def near_threshold(info, valid, bound):
    """Cells where a float64 evaluation of a compared quantity lies within ``bound`` of its threshold: |gaussian| against
    2 noise_std, the uniform field against the density map, |artifact| against amplitude / 2."""
    near = np.zeros(valid.shape, bool)
    if "gaussian64" in info:
        near |= np.abs(np.abs(info["gaussian64"]) - 2.0 * np.float64(info["noise_std"])) <= bound
    if "density" in info:
        near |= np.abs(info["spike_u"] - info["density"].astype(np.float64)) <= bound
    if "artifact64" in info:
        near |= np.abs(np.abs(info["artifact64"]) - 0.5 * np.float64(info["amplitude"])) <= bound
    return near & valid


def load_fixture(path):
    """(depth, valid, plan, params, fields, z) of one tests/golden/noise fixture; the sparse spike draws scattered to fields."""
    z = np.load(path)
    depth = z["clean_depth"]
    h, w = depth.shape
    valid = z["valid_mask"].astype(bool)
    sg = np.ones(h * w, np.int8)
    md = np.zeros(h * w, np.float64)
    sg[z["spike_index"]] = z["spike_sign"]
    md[z["spike_index"]] = z["spike_magnitude"]
    fields = {"gaussian": z["gaussian_field"], "uniform": z["uniform_field"], "sign": sg.reshape(h, w), "magnitude": md.reshape(h, w)}
    s = z["scalars"]      # std factor, density draw, artifact, amplitude factor, freq_a, freq_b, phase
    inten = float(z["intensity"])
    plan = {"sample": 0, "intensity": inten, "gaussian_std_factor": float(s[0]), "spike_density": float(s[1]) * inten,
            "blobs": [tuple(b) for b in z["blobs"]], "artifact": int(s[2]), "amplitude_factor": float(s[3]),
            "freq_a": float(s[4]), "freq_b": float(s[5]), "phase": float(s[6])}
    e = z["enable"]
    params = {"enable_gaussian": bool(e[0]), "enable_spikes": bool(e[1]), "enable_blobs": bool(e[2]), "enable_systematic": bool(e[3]),
              "complexity_correlation": float(z["complexity_correlation"]), "spike_magnitude_range": tuple(z["spike_magnitude_range"])}
    for k, on in (("gaussian", e[0]), ("uniform", e[1]), ("sign", e[1]), ("magnitude", e[1])):
        if not on:
            fields.pop(k)
    return depth, valid, plan, params, fields, z


EPS32 = float(np.finfo(np.float32).eps)


def check_outputs(out, depth, valid, info, ref_noisy64, ref_mask, ref_mag, ref_cls, noisy_bound, mag_bound, label=""):
    """The acceptance rule of the noise tests.  ``out`` = (noisy f32, mask bool, magnitude f32, classification i64) [h, w].
      - noisy: max |out - ref_noisy64| <= noisy_bound, separately over spike cells, blob cells and the remaining valid cells;
      - magnitude: |out - ref| <= mag_bound * |ref| at every cell;
      - mask / classification equal the reference's except at cells where a float64 evaluation of a compared quantity lies
        within noisy_bound of its threshold (``near_threshold``); those may number at most 0.1 % of the valid cells; every cell
        of a blob's area is marked (integer arithmetic: no exception);
      - invalid cells: input bits, unmarked, magnitude 0.
    Returns a report dict; raises AssertionError with ``label`` otherwise."""
    noisy, mask, mag, cls = out
    assert noisy.dtype == np.float32 and mask.dtype == bool and mag.dtype == np.float32 and cls.dtype == np.int64, label
    assert noisy.shape == mask.shape == mag.shape == cls.shape == depth.shape, label
    inv = ~valid
    assert np.array_equal(noisy.view(np.uint32)[inv], np.ascontiguousarray(depth, np.float32).view(np.uint32)[inv]), f"{label}: invalid cells changed"
    assert not mask[inv].any() and not mag[inv].any(), f"{label}: invalid cells labelled"
    assert np.array_equal(cls, np.where(mask, 2, 0)), f"{label}: classification is not 2 * noise_mask"
    report = {}
    nv = int(valid.sum())
    if nv == 0:
        return report
    spikes = info.get("spikes", np.zeros(valid.shape, bool))
    blobs = info["blob_cells"] & ~spikes
    err = np.abs(noisy.astype(np.float64) - ref_noisy64)
    for name, sel in (("spike", spikes), ("blob", blobs), ("quiet", valid & ~spikes & ~blobs)):
        if sel.any():
            report[name] = float(err[sel].max())
            print(f"{label} noisy_depth {name}: max err {report[name]:.3e} bound {noisy_bound:.3e} ({int(sel.sum())} cells)")
            assert report[name] <= noisy_bound, f"{label}: noisy_depth over {name} cells off by {report[name]:.3e} > {noisy_bound:.3e}"
    merr = np.abs(mag.astype(np.float64) - ref_mag.astype(np.float64))
    rel = float((merr / np.maximum(np.abs(ref_mag.astype(np.float64)), 1e-300))[ref_mag != 0].max()) if (ref_mag != 0).any() else 0.0
    print(f"{label} noise_magnitude: max rel err {rel:.3e} bound {mag_bound:.3e}")
    assert (merr <= mag_bound * np.abs(ref_mag.astype(np.float64))).all(), f"{label}: noise_magnitude rel err {rel:.3e} > {mag_bound:.3e}"
    near = near_threshold(info, valid, noisy_bound)
    diff = mask != ref_mask
    report.update(near=int(near.sum()), mask_diff=int(diff.sum()), magnitude_rel=rel)
    print(f"{label} noise_mask: {int(diff.sum())} differ, {int(near.sum())} near a threshold, {nv} valid")
    assert mask[info["blob_cells"]].all(), f"{label}: a blob cell is unmarked"
    assert not (diff & ~near).any(), f"{label}: noise_mask differs at {int((diff & ~near).sum())} cells away from every threshold"
    assert near.sum() <= 0.001 * nv, f"{label}: {int(near.sum())} cells near a threshold"
    assert np.array_equal(cls[~diff], ref_cls[~diff]), label
    return report


EXACT_FIXTURES = ("constant", "no_valid")      # every term is zero there: compared bit for bit, without exceptions


def check_fixture(out, path, c):
    """``check_outputs`` for a fixture: bounds from the reference's own float32 / float64 distance (c = BOUND_C); the
    constant-depth and no-valid-cell fixtures must match exactly."""
    depth, valid, plan, params, fields, z = load_fixture(path)
    if path.split("/")[-1][:-4] in EXACT_FIXTURES:
        assert np.array_equal(out[0].view(np.uint32), z["noisy_depth"].view(np.uint32)) and np.array_equal(out[1], z["noise_mask"])
        assert np.array_equal(out[2], z["noise_magnitude"]) and np.array_equal(out[3], z["classification"])
        assert out[3].dtype == np.int64 and out[1].dtype == bool
        return {}
    _, _, _, _, info = generate(depth, valid, plan, params, fields=fields)
    info.setdefault("blob_cells", np.zeros(valid.shape, bool))
    label = path.split("/")[-1]
    if not valid.any():
        noisy_bound = mag_bound = 0.0
    else:
        noisy_bound = c * float(np.abs(z["noisy_depth"].astype(np.float64) - z["noisy_depth64"])[valid].max())
        s32, s64 = float(z["std32"]), float(z["std64"])
        r = abs(s32 - s64) / s64 if s64 > 0 else 0.0
        mag_bound = c * (r + EPS32)
    return check_outputs(out, depth, valid, info, z["noisy_depth64"], z["noise_mask"], z["noise_magnitude"], z["classification"],
                         noisy_bound, mag_bound, label)
