"""numpy restatement of csrc/synthetic_noise.hip and of the counter-based generator of include/bgnn_noise.h.

``generate`` walks one tile through the four noise terms of the reference's ``SyntheticNoiseGenerator.generate`` with the
arithmetic the kernels use: per-tile scalars accumulated in float64 and rounded where numpy holds a float32, the windowed
standard deviation in float64 stored as float32, the reference's float32 / float64 mix in every term.  It takes the same plan
(scalars + blob list) and the same optional injected per-cell fields as ``bgnn_noise_generate``.  tests/test_host_noise.py pins
it against the reference's recorded outputs; tests/test_gpu_noise.py then uses it as the yardstick for the device's own draws.
The second half builds the tiles and the exact expectations of tests/test_gpu_noise_scale.py (training tile sizes).
"""
import functools

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
    filled = np.where(valid, depth, nanmean)
    ls = local_std(filled) if filled.size <= 1 << 16 else local_std_banded(filled)      # (the same bits: test_host_noise.py)
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


# ---- tiles at training sizes (tests/test_gpu_noise_scale.py; the inputs are checked by tests/test_host_noise.py) ---------------------
RUN = 256                # cells per run of the device's rank-select (one noise_apply workgroup)
STRIPS = 256             # strips of runs: one per thread of noise_finalize
STATS_STRIDE = 64 * 256  # cells one trip of the statistics passes covers (NOISE_NB1 workgroups of 256 threads)


def local_std_banded(filled, band=32, window=11, mode="edge", shift=0):
    """``local_std`` in bands of ``band`` rows, so that a 1024 x 1024 tile needs no [cells, 121] float64 array; the defaults
    give its bits.  ``window``, ``mode`` (numpy.pad) and ``shift`` (columns the window is moved to the right) restate it wrongly
    on purpose, for the checks that the complexity probe sees such a defect."""
    h, w = filled.shape
    r, n = window // 2, window * window
    p = np.pad(filled.astype(np.float64), ((r, r), (r - shift, r + shift)), mode=mode)
    out = np.empty((h, w), np.float32)
    for r0 in range(0, h, band):
        r1 = min(h, r0 + band)
        win = np.lib.stride_tricks.sliding_window_view(p[r0:r1 + 2 * r], (window, window)).reshape(r1 - r0, w, n)
        mean = win.sum(-1) / float(n)
        out[r0:r1] = np.sqrt(((win - mean[..., None]) ** 2).sum(-1) / float(n)).astype(np.float32)
    return out


def spike_density_map(ls, spike_density, complexity_correlation):
    """The density map of ``generate`` from a local_std map (float32 throughout)."""
    lmin, lmax = ls.min(), ls.max()
    cx = (ls - lmin) / (lmax - lmin) if lmax > lmin else np.zeros_like(ls)
    return np.float32(spike_density) * (np.float32(1) + np.float32(complexity_correlation) * (cx - np.float32(0.5)))


def run_counts(valid):
    """Valid cells of every run of RUN cells of a tile, row-major (the device's ``segcnt``)."""
    flat = np.asarray(valid, bool).ravel()
    return np.add.reduceat(flat.astype(np.int64), np.arange(0, flat.size, RUN))


def select_path(valid, k):
    """Where the device's rank-select meets the k-th valid cell: its run, its strip (``per`` runs per strip) and the categories
    the tests of the blob centres want covered."""
    c = run_counts(valid)
    nr = len(c)
    per = (nr + STRIPS - 1) // STRIPS
    run = int(np.searchsorted(np.cumsum(c), k, side="right"))
    strip = run // per
    strip_count = np.add.reduceat(c, np.arange(0, nr, per))
    return {"run": run, "strip": strip, "per": per, "runs": nr,
            "after_empty_strip": bool(strip > 0 and strip_count[strip - 1] == 0),
            "last_strip": strip == (nr - 1) // per,
            "not_first_run_of_strip": run % per != 0,
            "final_partial_run": bool(run == nr - 1 and valid.size % RUN != 0)}


def device_rank_select(valid, u):
    """noise_finalize's rank-select, step by step: a prefix over the strips, a walk over the runs of one strip, a walk over the
    cells of one run.  (row, col) like ``kth_valid_cell``, or None where the device leaves the blob unresolved."""
    flat = np.asarray(valid, bool).ravel()
    n, seg = flat.size, run_counts(valid)
    nr = len(seg)
    per = (nr + STRIPS - 1) // STRIPS
    pre = [0]
    for t in range(STRIPS):
        pre.append(pre[-1] + int(seg[t * per:min(t * per + per, nr)].sum()))
    nv = pre[STRIPS]
    if nv <= 0:
        return None
    k = min(max(int(u * float(nv)), 0), nv - 1)
    j = 0
    while j < STRIPS - 1 and pre[j + 1] <= k:
        j += 1
    left, sg = k - pre[j], j * per
    sg_end = min(sg + per, nr)
    while sg < sg_end - 1 and left >= seg[sg]:
        left -= int(seg[sg])
        sg += 1
    for i in range(sg * RUN, min(sg * RUN + RUN, n)):
        if flat[i]:
            if left == 0:
                return divmod(i, valid.shape[1])
            left -= 1
    return None


def centre_draws(valid, total, seed, each=4):
    """Blob-centre draws ``u`` for a tile: 0, nextafter(1, 0) and 1 (clamps to the last valid cell), then (k + 0.5) / n_valid
    for k = 0, n_valid - 1, n_valid // 2, the last cell before and the first cell of up to ``each`` + 2 strip boundaries (those
    after an empty strip and the last one first) and run boundaries inside a strip (the final run first), and random k up to
    ``total`` draws.  Returns (us, ks): ks[i] = the rank the device must resolve us[i] to."""
    nv = int(np.asarray(valid).sum())
    c = run_counts(valid)
    nr = len(c)
    per = (nr + STRIPS - 1) // STRIPS
    before = np.concatenate([[0], np.cumsum(c)[:-1]])            # valid cells before every run
    strip_count = np.add.reduceat(c, np.arange(0, nr, per))
    ks = [0, nv - 1, nv // 2]
    rng = np.random.default_rng(seed)

    def pick(cands, first):
        cands = [int(x) for x in cands]
        head = [x for x in first if x in cands]
        rest = [x for x in cands if x not in head]
        if len(rest) > each:
            rest = sorted(rng.choice(rest, each, replace=False).tolist())
        return head + rest

    strips = [j for j in range(1, len(strip_count)) if strip_count[j] > 0 and before[j * per] > 0]
    after_empty = [j for j in strips if strip_count[j - 1] == 0]
    for j in pick(strips, after_empty[:1] + strips[-1:]):
        ks += [int(before[j * per]) - 1, int(before[j * per])]
    runs = [r for r in range(nr) if r % per != 0 and c[r] > 0 and before[r] > 0]
    for r in pick(runs, runs[-1:]):
        ks += [int(before[r]) - 1, int(before[r])]
    ks += rng.integers(0, nv, max(0, total - 3 - len(ks))).tolist()
    one = float(np.nextafter(1.0, 0.0))
    us = [0.0, one, 1.0] + [(k + 0.5) / nv for k in ks]
    return us, [0, min(int(one * nv), nv - 1), nv - 1] + ks


def expected_unit_blobs(depth, valid, us):
    """What blobs of size 1 and magnitude draw 1.0 at intensity 1.0 must give, bit for bit: a size-1 blob covers its centre alone
    and adds exp(0) x depth_range there, once per blob in list order.  Returns noisy, mask, magnitude, depth_range."""
    depth = np.ascontiguousarray(depth, np.float32)
    noisy, mask, mag = depth.copy(), np.zeros(depth.shape, bool), np.zeros(depth.shape, np.float32)
    idx = np.flatnonzero(np.asarray(valid, bool).ravel())
    if len(idx) == 0:
        return noisy, mask, mag, np.float32(0)
    vd = depth.ravel()[idx]
    range32 = np.float32(vd.max()) - np.float32(vd.min())
    for u in us:
        i = idx[min(int(u * len(idx)), len(idx) - 1)]
        noisy.flat[i] = np.float32(np.float64(noisy.flat[i]) + np.float64(range32))
        mask.flat[i] = True
        mag.flat[i] = range32
    return noisy, mask, mag, range32


def _field(h, w, seed):
    from bathymetric_gnn_amd import synthetic
    return synthetic.synthetic_tile(h, w, seed, "V0")[0]


CENTRE_NAMES = ("260x253 0.9 valid", "17x16 full", "7x11 full", "300x517 0.01 valid", "300x517 rows 40..199 invalid", "64x64 no valid cell",
                "260x253 only the first cell", "260x253 only the last cell", "260x253 only the last partial run", "3x30000 0.5 valid",
                "512x512 V1", "1024x1024 V1")
SCALAR_NAMES = ("holes 1e6", "holes NaN", "valid among the last 300")


def centre_case(i):
    """(name, depth, valid, draws) of tile i of ``centre_tiles``; a tile without a valid cell still gets a list of draws."""
    name, depth, valid, total, _ = centre_tiles()[i]
    us = centre_draws(valid, total, 100 + i)[0] if valid.any() else [j / total for j in range(total)] + [1.0]
    return name, depth, valid, us


@functools.lru_cache(maxsize=None)
def centre_tiles():
    """[(name, depth, valid, draws wanted, categories its draws must reach)] of the blob-centre tests, in batch order: the
    272-cell and 77-cell tiles come before the large ones, whose runs then start at cell offsets of the batch that are a multiple
    of neither 256 nor 4."""
    from bathymetric_gnn_amd import synthetic
    rng = np.random.default_rng(20240)
    out = []

    def add(name, h, w, seed, valid, total, cats):
        out.append((name, _field(h, w, seed), np.ascontiguousarray(valid), total, cats))

    add("260x253 0.9 valid", 260, 253, 1, rng.random((260, 253)) < 0.9, 720, ("last_strip", "not_first_run_of_strip", "final_partial_run"))
    add("17x16 full", 17, 16, 2, np.ones((17, 16), bool), 24, ("final_partial_run",))
    add("7x11 full", 7, 11, 9, np.ones((7, 11), bool), 12, ("final_partial_run",))
    add("300x517 0.01 valid", 300, 517, 3, rng.random((300, 517)) < 0.01, 96, ("last_strip", "not_first_run_of_strip", "final_partial_run"))
    v = np.ones((300, 517), bool)
    v[40:200] = False
    add("300x517 rows 40..199 invalid", 300, 517, 4, v, 96, ("after_empty_strip", "last_strip", "not_first_run_of_strip", "final_partial_run"))
    add("64x64 no valid cell", 64, 64, 5, np.zeros((64, 64), bool), 8, ())
    for name, cells in (("first cell", [0]), ("last cell", [260 * 253 - 1]), ("last partial run", list(range(256 * 256 + 3, 260 * 253, 7)))):
        v = np.zeros(260 * 253, bool)
        v[cells] = True
        add(f"260x253 only the {name}", 260, 253, 6, v.reshape(260, 253), 16, ("last_strip", "final_partial_run") if cells[0] else ())
    add("3x30000 0.5 valid", 3, 30000, 7, rng.random((3, 30000)) < 0.5, 64, ("last_strip", "not_first_run_of_strip", "final_partial_run"))
    for side in (512, 1024):
        d, m, _ = synthetic.synthetic_tile(side, side, 8 + side, "V1")
        out.append((f"{side}x{side} V1", d, m, 96, ("last_strip", "not_first_run_of_strip")))
    return out


@functools.lru_cache(maxsize=None)
def scalar_tiles():
    """[(name, depth, valid)] for the per-tile scalars at 300 x 517 (workgroups of the statistics passes make 9 or 10 trips):
    a tile at -4000 m with centimetre relief (float32 holds it to 0.24 mm; a one-pass variance in float32 loses all of it),
    minimum and maximum in cells that only the last trip reads, invalid cells holding 1.0e6 / NaN; and a tile whose valid cells
    lie among its last 300 only."""
    from _conditioning import deep_tile
    h, w = 300, 517
    n = h * w
    from bathymetric_gnn_amd import synthetic
    relief = -4000.0 + 0.01 * (deep_tile(h, w, 11, "V0", depth=-4000.0)[0].astype(np.float64) + 4000.0)
    m = synthetic.synthetic_tile(h, w, 11, "V1")[1].copy()
    last_trip = (n - 1) // STATS_STRIDE * STATS_STRIDE
    relief.flat[last_trip + 2500] = relief.min() - 0.5
    relief.flat[n - 1] = relief.max() + 0.5
    m.flat[last_trip + 2500] = m.flat[n - 1] = True
    out = [("holes 1e6", np.where(m, relief, 1.0e6).astype(np.float32), m),
           ("holes NaN", np.where(m, relief, np.nan).astype(np.float32), m)]
    tail = np.zeros(n, bool)
    tail[n - 300:] = np.random.default_rng(12).random(300) < 0.5
    tail[n - 1] = True
    tail = tail.reshape(h, w)
    out.append(("valid among the last 300", np.where(tail, relief, 1.0e6).astype(np.float32), tail))
    return out


def longdouble_std32(depth, valid):
    """Two-pass population standard deviation of the valid cells in np.longdouble, rounded to float32."""
    v = np.asarray(depth)[np.asarray(valid, bool)].astype(np.longdouble)
    mean = v.sum() / np.longdouble(len(v))
    return np.float32(np.sqrt(((v - mean) ** 2).sum() / np.longdouble(len(v))))


@functools.lru_cache(maxsize=None)
def probe_tiles():
    """[(name, depth, valid)] of the complexity probe, the largest last."""
    from bathymetric_gnn_amd import synthetic
    out = []
    for h, w, seed in ((16, 16, 31), (17, 33, 32), (37, 19, 33), (3, 700, 34), (700, 3, 35), (1, 40, 36)):
        out.append((f"{h}x{w}", _field(h, w, seed), np.ones((h, w), bool)))
    d, m, _ = synthetic.synthetic_tile(48, 40, 37, "V1")
    d = d.copy()
    d[~m] = _field(48, 40, 38)[~m]
    d.flat[np.flatnonzero(~m.ravel())[3]] = np.inf
    out.append(("48x40 inf in an invalid cell", d, m))
    d, m, _ = synthetic.synthetic_tile(260, 253, 39, "V1")
    out.append(("260x253 NaN holes", np.where(m, d, np.float32(np.nan)), m))
    out.append(("260x253 1e6 holes", d, m))
    return out


PROBE_DENSITY, PROBE_CC = 0.005, 1.0
PROBE_PARAMS = {"enable_gaussian": False, "enable_spikes": True, "enable_blobs": False, "enable_systematic": False,
                "complexity_correlation": PROBE_CC, "spike_magnitude_range": (1.0, 5.0)}


def complexity_probe(depth, valid, c):
    """Makes every valid cell of a tile sensitive to its local_std: the injected uniform field is density x (1 + s delta), s = +1 /
    -1 on a chessboard and density the restatement's map, so that exactly the -1 squares spike.  ``delta`` = c x eps32 x
    (2 lmax / (lmax - lmin) + 2): a one-ulp float32 move of a cell's local_std, of lmin or of lmax moves the complexity by at most
    about eps32 x (lmax / (lmax - lmin) + 1) and the density relatively by twice that (2 c eps32 where the complexity is off).
    The sign and magnitude fields hold +-1 and multiples of 0.5 in [1, 5], so a spike's value is exact in float64.
    Returns (fields, delta, expected outputs of ``generate`` with these fields, its plan)."""
    h, w = depth.shape
    plan = {"sample": 0, "intensity": 1.0, "gaussian_std_factor": 0.0, "spike_density": PROBE_DENSITY, "blobs": [], "artifact": 0,
            "amplitude_factor": 0.0, "freq_a": 0.0, "freq_b": 0.0, "phase": 0.0}
    rr, cc = np.indices((h, w))
    fields = {"uniform": np.ones((h, w)), "sign": np.where((rr // 2 + cc) % 2, 1, -1).astype(np.int8),
              "magnitude": 1.0 + 0.5 * ((3 * rr + cc) % 9)}
    with np.errstate(invalid="ignore"):
        info = generate(depth, valid, plan, PROBE_PARAMS, fields=fields)[4]
        ls = info["local_std"]
        lmin, lmax = float(ls.min()), float(ls.max())
        ratio = lmax / (lmax - lmin) if lmax > lmin else 0.0
        delta = c * EPS32 * (2.0 * ratio + 2.0)
        s = np.where((rr + cc) % 2 == 0, 1.0, -1.0)
        fields["uniform"] = info["density"].astype(np.float64) * (1.0 + s * delta)
        ref = generate(depth, valid, plan, PROBE_PARAMS, fields=fields)
    return fields, delta, ref, (s < 0) & valid


# (h, w, tile seed of synthetic_tile V1, generator seed): own draws against the restatement, sample 0 each
OWN_CASES = ((260, 253, 3, 2024), (300, 517, 4, 77), (512, 512, 21, 5), (1024, 1024, 22, 6))
OWN_BATCH_SEED = 77
OWN_BATCH_SAMPLES = (1, 2, 3, 0, 4)          # the 300 x 517 tile keeps sample 0: it must come out as it does alone


@functools.lru_cache(maxsize=None)
def own_batch_tiles():
    """260 x 253, 17 x 16 (272 cells: the next tile starts misaligned), a tile without a valid cell, 300 x 517, 1 x 40."""
    from bathymetric_gnn_amd import synthetic
    t = lambda h, w, seed, variant="V1": synthetic.synthetic_tile(h, w, seed, variant)[:2]
    return [t(260, 253, 3), t(17, 16, 5), (t(64, 64, 1)[0], np.zeros((64, 64), bool)), t(300, 517, 4), t(1, 40, 6, "V0")]


def own_reference(depth, valid, plan, params, seed):
    """``generate`` on a device plan (data/synthetic_noise.py ``draw_plan``) and the bounds of the own-draw rule: noisy_depth
    c x eps32 x max |noisy|, magnitude c x eps32 (the caller multiplies by c)."""
    q = dict(plan)
    q["spike_density"] = float(plan["spike_density_draw"]) * plan["intensity"]
    q["artifact"] = ARTIFACTS.index(plan["artifact"])
    ref = generate(depth, valid, q, params, seed=seed)
    ref[4].setdefault("blob_cells", np.zeros(valid.shape, bool))
    scale = float(np.abs(ref[0][valid]).max()) if valid.any() else 0.0
    return ref, scale
