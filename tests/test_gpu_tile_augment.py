"""Training tiles gathered under the eight symmetries of the square on the GPU (include/bgnn_augment.h: ``bgnn_tile_gather``,
``TileStore.gather`` / ``batch(ops=...)``, ``Trainer(augment_geometry=True)``) against numpy's ``rot90`` / ``fliplr``.  The call moves
words and bytes, so every comparison here is a comparison of bits (int32 / uint8 views): nothing needs a tolerance."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_trainer import _config, _model, _stores, _tile

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5), (31, 33), (64, 64), (65, 63), (130, 70)]
INVERSE = [0, 3, 2, 1, 4, 5, 6, 7]
WORDS = ("depth", "unc", "labels", "difference")        # the four 4-byte planes, in the order of the call
SENT32, SENT8 = np.int32(-0x5A5A5A5B), np.uint8(0xA5)   # what the destinations hold before a call
PAD = 5                                                 # sentinel cells in front of, between and behind the tiles


def apply_op(t, op):
    return np.rot90(np.fliplr(t) if op >> 2 else t, op & 3)


def _planes(shape, tile):
    """The five planes of one source tile as bit patterns.  Every cell encodes (tile, row, column); the depth carries NaNs of distinct
    payloads (quiet and signalling, either sign) and both infinities, the labels are -1 / 0 / 1 / 2, the mask is any byte."""
    h, w = shape
    r, c = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    code = (tile << 16) + (r << 8) + c                                  # < 2^24: exact as float32
    depth = code.astype(np.float32).view(np.uint32).copy()
    flat = depth.reshape(-1)
    special = np.arange(0, flat.size, 7)
    kinds = [0x7FC00000, 0x7F800001, 0xFFC00000, 0xFF800001]
    flat[special] = [kinds[k % 4] + ((tile * 8191 + int(i)) & 0x3FFFF) * 2 for k, i in enumerate(special)]      # NaNs, payloads differ
    if flat.size > 3:
        flat[1], flat[3] = 0x7F800000, 0xFF800000                          # +inf, -inf
    return {"depth": depth.view(np.int32), "unc": (code + 0.5).astype(np.float32).view(np.int32),
            "labels": ((code * 7 + tile) % 4 - 1).astype(np.int32), "difference": (-code).astype(np.float32).view(np.int32),
            "mask": ((code * 13 + 5) % 251).astype(np.uint8)}


def _source_store(shapes, skip=()):
    """Flat source planes of the tiles ``shapes`` with PAD cells of filler around each: ``(planes, offsets, tiles)``."""
    tiles = [_planes(s, k + 1) for k, s in enumerate(shapes)]
    offsets, at = [], PAD
    for s in shapes:
        offsets.append(at)
        at += s[0] * s[1] + PAD
    planes = {}
    for name in WORDS + ("mask",):
        if name in skip:
            continue
        flat = np.full(at, 77, np.uint8 if name == "mask" else np.int32)
        for off, t in zip(offsets, tiles):
            flat[off:off + t[name].size] = t[name].ravel()
        planes[name] = flat
    return planes, offsets, tiles


def _raw_gather(src, dst, entries, src_cells=None, dst_cells=None, ws=None, ws_bytes=None, n=None, n_planes=4, src_list=None,
                dst_list=None, null=()):
    """``bgnn_tile_gather`` itself on dicts of device tensors (a missing word plane: a NULL pair): the return code.  ``null``: which
    of ctx / src / dst / entries / ws to pass as NULL."""
    from bathymetric_gnn_amd import runtime as rt
    ctx = rt.get_context(torch.device("cuda:0"))
    table = np.array([tuple(e) + (0,) for e in entries], dtype=rt.TILE_ENTRY_DTYPE).reshape(-1)
    n = len(table) if n is None else n
    need = int(ctx.lib.bgnn_tile_gather_workspace_bytes(max(len(table), 1)))
    if ws is None:
        ws = torch.empty(need // 8, dtype=torch.int64, device="cuda")
    some = next(iter(src.values())), next(iter(dst.values()))
    addr = lambda d, k: None if d.get(k) is None else d[k].data_ptr()
    s = src_list if src_list is not None else [addr(src, k) for k in WORDS]
    d = dst_list if dst_list is not None else [addr(dst, k) for k in WORDS]
    s_arr, d_arr = (C.c_void_p * len(s))(*s), (C.c_void_p * len(d))(*d)
    ctx.begin()
    rc = ctx.lib.bgnn_tile_gather(None if "ctx" in null else ctx.handle, None if "src" in null else s_arr, None if "dst" in null else d_arr,
                                  n_planes, rt.ptr(src.get("mask")), rt.ptr(dst.get("mask")),
                                  some[0].numel() if src_cells is None else src_cells, some[1].numel() if dst_cells is None else dst_cells,
                                  C.c_void_p(table.ctypes.data) if len(table) and "entries" not in null else None, n,
                                  None if "ws" in null else C.c_void_p(ws) if isinstance(ws, int) else rt.ptr(ws),
                                  C.c_size_t(need if ws_bytes is None else ws_bytes))
    ctx.end()
    return rc


def _sentinels(names, cells):
    return {k: torch.full((cells,), int(SENT8 if k == "mask" else SENT32), dtype=torch.uint8 if k == "mask" else torch.int32, device="cuda")
            for k in names}


def _check_gather(shapes, picks, skip=(), order=None):
    """Gather ``picks`` = [(tile, op), ...] of the source tiles ``shapes``; destinations PAD apart, laid out in ``order`` (a
    permutation of the entries: entry k takes the ``order[k]``-th place).  Everything against numpy, sentinel cells included."""
    planes, offsets, tiles = _source_store(shapes, skip)
    order = list(range(len(picks))) if order is None else order
    cells = [shapes[t][0] * shapes[t][1] for t, _ in picks]
    place = {}                                                          # position in the destination -> entry
    for k, o in enumerate(order):
        place[o] = k
    dst_at, at = [0] * len(picks), PAD
    for o in range(len(picks)):
        dst_at[place[o]] = at
        at += cells[place[o]] + PAD
    src = {k: torch.from_numpy(v).cuda() for k, v in planes.items()}
    dst = _sentinels(planes, at)
    entries = [(offsets[t], dst_at[k], shapes[t][0], shapes[t][1], op) for k, (t, op) in enumerate(picks)]
    assert _raw_gather(src, dst, entries) == 0
    for name in planes:
        want = np.full(at, SENT8 if name == "mask" else SENT32, planes[name].dtype)
        for k, (t, op) in enumerate(picks):
            want[dst_at[k]:dst_at[k] + cells[k]] = apply_op(tiles[t][name], op).ravel()
        got = dst[name].cpu().numpy()
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"{name}: {bad.size} cells differ, first at {bad[:5].tolist()} (entries {entries})"
    for name in skip:
        assert name not in dst
    return src, dst, entries


# ---- 1. the kernel against numpy ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_all_eight_ops_of_one_tile(shape, gpu_device):
    _check_gather([shape], [(0, op) for op in range(8)])


def test_every_shape_in_one_call_without_uncertainty(gpu_device):
    picks = [(t, (3 * t + k) % 8) for t in range(len(SHAPES)) for k in range(2)]
    assert {op for _, op in picks} == set(range(8))
    _check_gather(SHAPES, picks, skip=("unc",))


def test_the_byte_plane_alone_past_2_to_the_32_cells(gpu_device):
    """Cell offsets are 64-bit: one tile read from beyond cell 2^32 of a byte store and written beyond cell 2^32 of another (an
    offset cut to 32 bits would land in the stores' first cells, which are watched)."""
    h, w, op = 70, 65, 1
    base = 2 ** 32 + 9
    tile = _planes((h, w), 3)["mask"]
    src = torch.empty(base + h * w + PAD, dtype=torch.uint8, device="cuda")
    dst = torch.empty(base + 4 + h * w + PAD, dtype=torch.uint8, device="cuda")
    src[base - PAD:] = 77
    src[base:base + h * w] = torch.from_numpy(tile.ravel()).cuda()
    dst[:4096] = int(SENT8)
    dst[base - 4096:] = int(SENT8)
    assert _raw_gather({"mask": src}, {"mask": dst}, [(base, base + 4, h, w, op)], n_planes=0, src_list=[], dst_list=[]) == 0
    got = dst[base - 4096:].cpu().numpy()
    want = np.full(got.size, SENT8, np.uint8)
    want[4096 + 4:4096 + 4 + h * w] = apply_op(tile, op).ravel()
    assert np.array_equal(got, want)
    assert bool((dst[:4096] == int(SENT8)).all())                     # (where a truncated 32-bit offset would have landed)


# ---- 2. one source, several entries ------------------------------------------------------------------------------------------
def test_one_source_tile_named_by_several_entries(gpu_device):
    picks = [(0, 3), (1, 5), (0, 0), (0, 6), (1, 5), (0, 3)]
    _check_gather([(65, 63), (9, 40)], picks, order=[4, 0, 5, 2, 1, 3])


# ---- 3. round trip -------------------------------------------------------------------------------------------------------------
def test_round_trip_through_the_inverse(gpu_device):
    shape = (65, 63)
    src, mid, entries = _check_gather([shape], [(0, op) for op in range(8)])
    back = _sentinels(mid, mid["depth"].numel())
    h, w = shape
    again = [(e[1], e[1], w if op & 1 else h, h if op & 1 else w, INVERSE[op]) for op, e in enumerate(entries)]
    assert _raw_gather(mid, back, again) == 0
    for name in mid:
        want = src[name][PAD:PAD + h * w]
        got = back[name]
        for e in entries:
            assert torch.equal(got[e[1]:e[1] + h * w], want), (name, e)
        assert int((got == int(SENT8 if name == "mask" else SENT32)).sum()) >= got.numel() - 8 * h * w


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_destinations_untouched(gpu_device):
    from bathymetric_gnn_amd import runtime as rt
    lib = rt.load_library()
    planes, offsets, _ = _source_store([(6, 9)])
    src = {k: torch.from_numpy(v).cuda() for k, v in planes.items()}
    cells = src["depth"].numel()
    dst = _sentinels(planes, 100)
    ws = torch.empty(64, dtype=torch.int64, device="cuda")
    good = (offsets[0], 3, 6, 9, 1)
    ptrs = lambda d: [d[k].data_ptr() for k in WORDS]

    def refused(what, **kw):
        entries = kw.pop("entries", [good])
        s, d = kw.pop("src", src), kw.pop("dst", dst)
        rc = _raw_gather(s, d, entries, **{**dict(ws=ws, src_cells=cells, dst_cells=100), **kw})
        assert rc == rt.ERR_INVALID, (what, rc, lib.bgnn_last_error())
        torch.cuda.synchronize()
        for k, t in dst.items():
            assert bool((t == int(SENT8 if k == "mask" else SENT32)).all()), (what, k)

    for op in (-1, 8):
        refused(f"op {op}", entries=[good[:4] + (op,)])
    refused("h 0", entries=[(offsets[0], 3, 0, 9, 1)])
    refused("w 0", entries=[(offsets[0], 3, 6, 0, 1)])
    refused("source past the store", entries=[(cells - 53, 3, 6, 9, 1)])
    refused("destination past the store", entries=[(offsets[0], 47, 6, 9, 1)])
    refused("the second entry", entries=[good, (offsets[0], 60, 6, 9, 9)])
    refused("negative source", entries=[(-1, 3, 6, 9, 1)])
    refused("negative destination", entries=[(offsets[0], -1, 6, 9, 1)])
    refused("half a pair", src_list=ptrs(src)[:2] + [None] + ptrs(src)[3:])
    refused("half a pair", dst_list=ptrs(dst)[:1] + [None] + ptrs(dst)[2:])
    refused("half the byte pair", src={k: v for k, v in src.items() if k != "mask"})
    refused("five planes", n_planes=5, src_list=ptrs(src) + [src["depth"].data_ptr()], dst_list=ptrs(dst) + [dst["depth"].data_ptr()])
    for name in ("ctx", "src", "dst", "entries", "ws"):
        refused(f"NULL {name}", null=(name,))
    refused("misaligned workspace", ws=ws.data_ptr() + 8)
    refused("small workspace", ws_bytes=255)
    assert cells == 64
    refused("destination on a source", dst_list=[src["depth"].data_ptr() + 4 * (cells - 60)] + ptrs(dst)[1:], dst_cells=60)
    refused("byte destination on a byte source", dst={**dst, "mask": src["mask"]}, dst_cells=64)
    # n_entries == 0: accepted, and nothing is written
    assert _raw_gather(src, dst, [], ws=ws, src_cells=cells, dst_cells=100) == 0
    assert _raw_gather(src, dst, [good], n=0, ws=ws, src_cells=cells, dst_cells=100) == 0
    torch.cuda.synchronize()
    for k, t in dst.items():
        assert bool((t == int(SENT8 if k == "mask" else SENT32)).all()), k
    # and the same arguments, accepted, do write (the refusals above were not refusals of something else)
    assert _raw_gather(src, dst, [good], ws=ws, src_cells=cells, dst_cells=100) == 0
    assert int((dst["depth"] != int(SENT32)).sum()) == 54 and int((dst["labels"] != int(SENT32)).sum()) == 54


# ---- 5. batch(ops) equals a pre-turned store ---------------------------------------------------------------------------------
A_SHAPES = [(40, 40), (40, 40), (24, 56), (9, 9)]
A_OPS = np.array([1, 6, 3, 7], np.int8)
A_RES = [(0.5, 1.0), (0.5, 1.0), (2.0, 1.0), (0.25, 0.5)]


def _a_tiles():
    """depth, mask, uncertainty, labels (-1 where invalid), difference of the four tiles of store A; every tile has invalid cells."""
    rng = np.random.default_rng(23)
    out = []
    for k, (h, w) in enumerate(A_SHAPES):
        d, m, _ = _tile(h, w, 60 + k, "V1" if h > 9 else "V0")           # (the holes of V1 leave a 9 x 9 tile without a valid cell)
        m = m.copy()
        m[1:3, 2:5] = False
        m[h - 2, 0] = False
        lab = rng.choice(np.array([0, 1, 2], np.int32), size=(h, w), p=(0.7, 0.1, 0.2)).astype(np.int32)
        lab[~m] = -1
        out.append({"depth": d.astype(np.float32), "mask": m, "unc": rng.random((h, w), dtype=np.float32), "labels": lab,
                    "difference": rng.normal(0.0, 0.3, (h, w)).astype(np.float32)})
        assert 0 < (~m).sum() < m.size - 2
    return out


def _turned(tiles):
    return [{k: np.ascontiguousarray(apply_op(v, int(op))) for k, v in t.items()} for t, op in zip(tiles, A_OPS)]


def _truth_store(tiles, res):
    from bathymetric_gnn_amd.training import TileStore
    flat = lambda k, dt: torch.from_numpy(np.concatenate([np.ascontiguousarray(t[k], dt).ravel() for t in tiles])).cuda()
    hw = np.array([t["depth"].shape for t in tiles], np.int32)
    return TileStore("ground_truth", hw, np.array(res, np.float64), flat("depth", np.float32), flat("mask", np.uint8), flat("unc", np.float32),
                     labels=flat("labels", np.int32), difference=flat("difference", np.float32))


def _noise_store(tiles, res):
    from bathymetric_gnn_amd.training import TileStore
    return TileStore.from_tiles([t["depth"] for t in tiles], [t["mask"] for t in tiles], None, res, seed=3)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_batch(a, b):
    (ga, ta), (gb, tb) = a, b
    assert ga.num_nodes == gb.num_nodes > 0 and ga.num_edges == gb.num_edges > 0
    assert np.array_equal(ga._hw, gb._hw)
    for k in ("x", "edge_index", "edge_attr"):
        assert torch.equal(_bits(getattr(ga, k)), _bits(getattr(gb, k))), k
    assert sorted(ta) == sorted(tb) == ["class_labels", "correction_targets", "noise_mask"]
    for k in ta:
        assert ta[k].dtype == tb[k].dtype and torch.equal(_bits(ta[k]), _bits(tb[k])), k


@pytest.mark.parametrize("kind,epoch", [("ground_truth", 0), ("synthetic", 0), ("synthetic", 3)])
def test_batch_with_ops_equals_a_store_turned_beforehand(kind, epoch, gpu_device):
    tiles = _a_tiles()
    res_b = [r[::-1] if op & 1 else r for r, op in zip(A_RES, A_OPS)]
    make = _truth_store if kind == "ground_truth" else _noise_store
    A, B = make(tiles, A_RES), make(_turned(tiles), res_b)
    assert len(A) == len(B) == 4 and not A.uniform
    for idx in ([2, 0, 3, 1], [1, 2], [3]):
        _same_batch(A.batch(idx, epoch, ops=A_OPS[idx]), B.batch(idx, epoch))
    # the table of the gather itself, and the identity through it
    hw, res, planes = A.gather([2, 3], A_OPS[[2, 3]])
    assert hw.tolist() == [[56, 24], [9, 9]] and res.tolist() == [[1.0, 2.0], [0.5, 0.25]]
    for k in ("depth", "mask", "unc", "labels", "difference"):
        want = getattr(B, k)
        assert (planes[k] is None) == (want is None)
        if want is not None:
            assert torch.equal(_bits(planes[k]), _bits(want[int(B.offsets[2]):int(B.offsets[4])])), k
    idx = [3, 1, 0, 2]
    _same_batch(A.batch(idx, epoch), A.batch(idx, epoch, ops=np.zeros(4, np.int8)))
    differs = A.batch([2], epoch, ops=[1])[0]
    assert differs._hw.tolist() == [[56, 24]] and A.batch([2], epoch)[0]._hw.tolist() == [[24, 56]]
    with pytest.raises(ValueError):
        A.batch([0, 1], epoch, ops=[0])
    with pytest.raises(ValueError):
        A.batch([0], epoch, ops=[8])


IDENTITY_CASES = {"ragged": ([(65, 63), (9, 40), (40, 40), (40, 40), (2, 2)], [[4, 0, 2, 1, 3], [1, 1], [3]]),
                  "uniform": ([(40, 40)] * 3, [[2, 0]])}


@pytest.mark.parametrize("with_unc", [True, False], ids=["unc", "no_unc"])
@pytest.mark.parametrize("case", list(IDENTITY_CASES))
def test_gather_without_ops_is_the_stored_cells_in_order(case, with_unc, gpu_device):
    """``gather(idx, None)`` -- the path of every ``batch`` without ops -- against slices of a host copy of the store's planes, not
    against the library: tile ``i`` of a batch is the cells ``offsets[i] .. offsets[i + 1] - 1`` of every plane, in the order of
    ``idx``, bit for bit.  The float planes hold NaNs of distinct payloads and both infinities in invalid cells: the words are
    moved, not interpreted.  The shapes reach every branch of the 64 x 64-block kernel (a tile wider and one narrower than a block,
    partial blocks, a tile smaller than a wave) and both kinds of store (ragged, uniform)."""
    from bathymetric_gnn_amd.training import TileStore
    shapes, batches = IDENTITY_CASES[case]
    tiles = [_planes(s, k + 1) for k, s in enumerate(shapes)]
    for t in tiles:                                       # invalid where the depth is NaN or infinite; NaNs in the other planes too
        flat = {k: v.reshape(-1) for k, v in t.items()}
        bad = np.arange(0, flat["mask"].size, 7)
        flat["mask"][bad], flat["mask"][[1, 3]] = 0, 0
        flat["unc"].view(np.uint32)[bad] = 0xFFC00000 + bad
        flat["difference"].view(np.uint32)[bad[::2]] = 0x7F800001 + bad[::2]
        flat["difference"].view(np.uint32)[[1, 3]] = 0xFF800000, 0x7F800000
    built = {k: np.concatenate([t[k].ravel() for t in tiles]) for k in WORDS + ("mask",) if with_unc or k != "unc"}
    dev = {k: torch.from_numpy(v).cuda() for k, v in built.items()}
    word = lambda k, dt: None if k not in dev else dev[k].view(dt)
    store = TileStore("ground_truth", np.array(shapes, np.int32), np.ones((len(shapes), 2)), word("depth", torch.float32), dev["mask"],
                      word("unc", torch.float32), labels=dev["labels"], difference=word("difference", torch.float32))
    assert store.uniform == (case == "uniform") and (store.unc is None) == (not with_unc)
    host = {k: None if getattr(store, k) is None else _bits(getattr(store, k)).cpu().numpy() for k in WORDS + ("mask",)}
    off = store.offsets
    assert off.tolist() == np.concatenate([[0], np.cumsum([h * w for h, w in shapes])]).tolist()
    for k, v in built.items():
        assert np.array_equal(host[k], v), k
    depth, invalid = host["depth"].view(np.float32), host["mask"] == 0
    assert np.isnan(depth[invalid]).sum() > 2 and np.isposinf(depth[invalid]).any() and np.isneginf(depth[invalid]).any()
    assert len(np.unique(host["depth"][invalid])) > invalid.sum() // 2          # (the payloads differ)
    for idx in batches:
        hw, res, planes = store.gather(idx, None)
        assert hw.tolist() == [list(shapes[i]) for i in idx] and res.tolist() == [[1.0, 1.0]] * len(idx)
        assert sorted(planes) == sorted(WORDS + ("mask",))
        for k in planes:
            if host[k] is None:
                assert planes[k] is None and k == "unc" and not with_unc
                continue
            want = np.concatenate([host[k][off[i]:off[i + 1]] for i in idx])
            got = _bits(planes[k]).cpu().numpy()
            assert got.dtype == want.dtype and np.array_equal(got, want), (k, idx)


# ---- 6. the Trainer --------------------------------------------------------------------------------------------------------------
def _run(tmp, name, epochs=2, seed=4, **kw):
    from bathymetric_gnn_amd.training import Trainer
    flags = kw.pop("flags", None)
    cfg = _config(epochs=epochs) if flags is None else _config(epochs=epochs, augment_rotations=flags, augment_flips=flags)
    t = Trainer(cfg, _model("GAT"), *_stores(), output_dir=tmp / name, seed=seed, **kw)
    return t, copy.deepcopy(t.train())


def _same_weights(a, b):
    sa, sb = a.model.state_dict(), b.model.state_dict()
    return list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


@pytest.fixture(scope="module")
def runs(tmp_path_factory, gpu_device):
    """The unaugmented run and the augmented one (both flags), two epochs each, shared by the tests below."""
    tmp = tmp_path_factory.mktemp("augment")
    return tmp, _run(tmp, "plain"), _run(tmp, "turned", flags=True, augment_geometry=True)


def test_trainer_identity_through_the_new_path(runs):
    tmp, (plain, h_plain), _ = runs
    assert plain.augment_geometry is False
    ident, h = _run(tmp, "identity", flags=False, augment_geometry=True)
    assert ident.augment_geometry is True and not ident.augment_plan(0).any() and not ident.augment_plan(1).any()
    assert h == h_plain and all(len(v) == 2 and all(np.isfinite(v)) for v in h.values())
    assert _same_weights(ident, plain)


def test_trainer_augmented_runs_are_reproducible_and_differ(runs):
    tmp, (plain, h_plain), (turned, h_turned) = runs
    plan = [turned.augment_plan(e) for e in (0, 1)]
    assert all(p.shape == (6,) and p.dtype == np.int8 for p in plan) and any(p.any() for p in plan)
    again, h = _run(tmp, "turned_again", flags=True, augment_geometry=True)
    assert h == h_turned and _same_weights(again, turned)
    assert not _same_weights(turned, plain) and h_turned["train_loss"] != h_plain["train_loss"]
    assert h_turned["train_loss"][0] != h_plain["train_loss"][0]       # already the first epoch saw other tiles
    assert [p[0].tolist() for p in turned.step_plan(1)] == [p[0].tolist() for p in plain.step_plan(1)]      # the plan is as it was


def test_trainer_resumed_run_continues_the_augmented_one(runs):
    from bathymetric_gnn_amd.training import Trainer
    tmp, _, (turned, h_turned) = runs
    first, h1 = _run(tmp, "first", epochs=1, flags=True, augment_geometry=True)
    assert h1 == {k: v[:1] for k, v in h_turned.items()}
    second = Trainer(_config(epochs=2, augment_rotations=True, augment_flips=True), _model("GAT", seed=99), *_stores(),
                     output_dir=tmp / "second", seed=4, augment_geometry=True)
    ckpt = second.resume(tmp / "first" / "final_model.pt")
    assert "augment" not in " ".join(ckpt) and second.current_epoch == 0
    h = second.train()
    assert h == h_turned and _same_weights(second, turned)
    sa, sb = turned.optimizer.state_dict(), second.optimizer.state_dict()
    for i in sa["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sa["state"][i][k], sb["state"][i][k]), (i, k)


def test_trainer_validates_on_unturned_tiles(runs):
    """The last validation epoch replayed by hand on the store as it lies (no ops), with the weights the run ended with."""
    _, _, (turned, h_turned) = runs
    model, crit = turned.model, turned.criterion
    model.eval()
    total, correct, nodes = 0.0, 0, 0
    with torch.no_grad():
        for idx, seed in turned.step_plan(1, validation=True):
            assert seed is None
            g, t = turned.val_store.batch(idx, 1)
            assert g._hw.tolist() == [[32, 40]] * len(idx)
            out = model(g)
            losses = crit(out, t)
            total += losses["total"].item() * g.num_nodes
            correct += (out["predicted_class"] == t["class_labels"]).sum().item()
            nodes += g.num_nodes
    assert h_turned["val_loss"][1] == total / nodes and h_turned["val_acc"][1] == correct / nodes
    # ... and a turned validation batch would not have given that loss
    with torch.no_grad():
        g, t = turned.val_store.batch([0, 1], 1, ops=[1, 1])
        other = crit(model(g), t)["total"].item()
    assert g._hw.tolist() == [[40, 32]] * 2 and other != total / nodes
