"""Hostile foreign graphs for ``tests/test_gpu_foreign_scale.py``: what a ``Data`` assembled elsewhere may look like, shaped so
that every branch of the generic CSR build (graph_build.hip), of the transposed index (gat_backward.hip) and of the CSR forms of
the aggregate and backward kernels is reached.  Host numpy only; every property is asserted before the graph is returned."""
import numpy as np

PINNED_DEGREES = (15, 16, 17, 32, 33)    # around AGG_MAXDEG = 16 (register array | three-pass loop) and around 32
BOUNDARY = {2047: 16, 2048: 17, 2049: 33}  # ids on both sides of the first scan-chunk boundary (SCAN_CHUNK = 2048) -> in-degree
HUB, FAN = 5, 7                          # the node with LONG in-edges, the node with LONG out-edges
SINK, SOURCE = 8, 9                      # in-edges only, out-edges only
LONG = 1000
N_ISOLATED = 10
N_PARALLEL = 200
N_SELF_LOOPS = 64


def in_degree(ei, N):
    """In-degree as the CSR build counts it: explicit self loops do not count."""
    keep = ei[0] != ei[1]
    return np.bincount(ei[1, keep], minlength=N)


def foreign_graph(N, mean_deg=8, seed=0, self_loops=True, long_lists=LONG):
    """(x [N, 7] f32, edge_index [2, E] i64, edge_attr [E, 3] f32) of a random directed graph on ``N`` nodes:

    - ~``mean_deg`` x N random one-way edges, the whole edge array in random order (a row's edge ids are spread over all of it);
    - ``pinned(N)``: nodes whose in-degree is exactly 15, 16, 17, 32 and 33 (ids 11 .. 15), and -- where N leaves room before the
      isolated tail -- ids 2047 / 2048 / 2049 with 16 / 17 / 33 in-edges, on both sides of a scan-chunk boundary;
    - node 5 has exactly ``long_lists`` in-edges from distinct sources, node 7 exactly ``long_lists`` out-edges to distinct targets;
    - 200 repeated (parallel) edges; with ``self_loops`` 64 explicit self loops, three of them on pinned rows (the CSR drops
      them, so a 16-edge row with a self loop still has 16 entries);
    - node 8 has in-edges only, node 9 out-edges only, the last 10 nodes are isolated.
    ``long_lists = 0`` (tiny graphs) leaves the two long lists and the parallel edges' count to chance."""
    rng = np.random.default_rng(seed)
    A = N - N_ISOLATED                                            # nodes [0, A) may carry edges
    assert A >= 64, N
    pin = pinned(N)
    fixed_in = np.array(sorted(set(pin) | {HUB, SOURCE}))          # their in-edges are placed by hand
    no_dup_dst = fixed_in

    def sources(k, exclude, distinct=False):
        pool = np.setdiff1d(np.arange(A), np.array(list(exclude) + [SINK]))
        return rng.choice(pool, size=k, replace=not distinct)

    parts = []
    E0 = int(N * mean_deg)
    s, d = rng.integers(0, A, E0), rng.integers(0, A, E0)
    keep = (s != d) & ~np.isin(d, fixed_in) & (s != SINK) & (s != FAN)
    parts.append(np.stack([s[keep], d[keep]]))
    for node, deg in pin.items():
        parts.append(np.stack([sources(deg, [node, FAN]), np.full(deg, node)]))
    if long_lists:
        assert A - len(fixed_in) - 3 >= long_lists, (N, long_lists)
        parts.append(np.stack([sources(long_lists, [HUB, FAN], distinct=True), np.full(long_lists, HUB)]))
        targets = rng.choice(np.setdiff1d(np.arange(A), np.concatenate([fixed_in, [FAN]])), size=long_lists, replace=False)
        parts.append(np.stack([np.full(long_lists, FAN), targets]))
    parts.append(np.stack([sources(3, [FAN]), np.full(3, SINK)]))
    free = np.setdiff1d(np.arange(A), np.concatenate([fixed_in, [FAN, SINK]]))
    parts.append(np.stack([np.full(3, SOURCE), rng.choice(free, size=3, replace=False)]))
    ei = np.concatenate(parts, axis=1)
    cand = np.flatnonzero(~np.isin(ei[1], no_dup_dst) & (ei[0] != FAN))
    ei = np.concatenate([ei, ei[:, rng.choice(cand, size=N_PARALLEL, replace=False)]], axis=1)
    if self_loops:
        others = np.setdiff1d(np.arange(A), np.array([SINK, SOURCE, FAN] + list(pin)))
        loops = np.concatenate([[12, 13, 15], rng.choice(others, size=N_SELF_LOOPS - 3, replace=False)])
        ei = np.concatenate([ei, np.stack([loops, loops])], axis=1)
    ei = np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])]).astype(np.int64)
    E = ei.shape[1]
    x = rng.standard_normal((N, 7)).astype(np.float32)
    ea = rng.standard_normal((E, 3)).astype(np.float32)

    # ---- the properties the tests rely on ----
    real = ei[0] != ei[1]
    deg_in = in_degree(ei, N)
    deg_out = np.bincount(ei[0, real], minlength=N)
    for node, deg in pin.items():
        assert deg_in[node] == deg, (node, deg_in[node], deg)
    assert set(PINNED_DEGREES) <= set(pin.values())
    if long_lists:
        assert deg_in[HUB] == long_lists == len(np.unique(ei[0, real & (ei[1] == HUB)])) and deg_in.max() == long_lists
        assert deg_out[FAN] == long_lists == len(np.unique(ei[1, real & (ei[0] == FAN)])) and deg_out.max() == long_lists
        ids = np.flatnonzero(ei[1] == HUB)                         # random edge order: the hub's edge ids span the array
        assert ids.max() - ids.min() > E // 2
    key = ei[0, real] * N + ei[1, real]
    assert len(key) - len(np.unique(key)) >= N_PARALLEL            # parallel edges
    assert np.isin(key, ei[1, real] * N + ei[0, real]).mean() < 0.1  # mostly one-way
    assert int((~real).sum()) == (N_SELF_LOOPS if self_loops else 0)
    assert deg_in[SINK] > 0 and deg_out[SINK] == 0 and deg_out[SOURCE] > 0 and deg_in[SOURCE] == 0
    assert not deg_in[A:].any() and not deg_out[A:].any() and ei.max() < A
    assert (deg_in[:A] == 0).sum() >= 1                            # (SOURCE at least) rows of length 0 inside the graph
    return x, ei, ea


def pinned(N):
    """{node id: exact in-degree} of ``foreign_graph(N, ...)``."""
    pin = {11 + i: d for i, d in enumerate(PINNED_DEGREES)}
    pin.update({i: d for i, d in BOUNDARY.items() if i < N - N_ISOLATED})
    return pin


def keep_target_order(ei, seed):
    """A permutation of the edges that keeps the relative order of edges sharing a target (so every CSR row, sorted by edge id,
    is unchanged): the targets' groups are laid out in a random interleave, each group's edges in their old order."""
    rng = np.random.default_rng(seed)
    E = ei.shape[1]
    by_target = np.argsort(ei[1], kind="stable")                   # old edge ids, grouped by target, ascending inside a group
    slots = np.argsort(ei[1][rng.permutation(E)], kind="stable")   # new positions, grouped by target the same way
    perm = np.empty(E, np.int64)
    perm[slots] = by_target                                        # new edge k is old edge perm[k]
    assert np.array_equal(np.sort(perm), np.arange(E)) and (perm != np.arange(E)).mean() > 0.9
    first = np.argsort(ei[1, perm], kind="stable")
    assert np.array_equal(perm[first], by_target)                  # every target's edges in their old order
    return perm


def replicate(x, ei, ea, copies, seed):
    """``copies`` disjoint copies of a graph as one graph: copy c's nodes are c N .. (c + 1) N - 1, and the copies' edge lists are
    merged by a random interleave that keeps each copy's internal order, so every copy's rows (sorted by edge id) hold copy 0's
    neighbours in copy 0's order."""
    N, E = x.shape[0], ei.shape[1]
    rng = np.random.default_rng(seed)
    owner = rng.permutation(np.repeat(np.arange(copies, dtype=np.int16), E))
    pos = np.argsort(owner, kind="stable")                         # positions of copy 0's edges (ascending), then copy 1's, ...
    big_ei = np.empty((2, copies * E), np.int64)
    big_ea = np.empty((copies * E, ea.shape[1]), np.float32)
    for c in range(copies):
        p = pos[c * E:(c + 1) * E]
        big_ei[:, p] = ei + c * N
        big_ea[p] = ea
    assert (np.diff(pos.reshape(copies, E), axis=1) > 0).all()
    return np.tile(x, (copies, 1)), big_ei, big_ea
