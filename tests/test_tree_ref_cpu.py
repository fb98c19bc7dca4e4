"""The shortest-path tree reference (tests/tree_ref.py) against the oracle's arithmetic and the
reference's own test graph, the definition's tie rules on a hand graph, the suffix case, the
host-only sg_tree_path, and the conditions the GPU cases' inputs must meet (test_tree_gpu.py),
checked here so that the inputs qualify by the reference alone.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import tree_cases as TC
import tree_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(O, g, nodes=None, rows=None):
    nodes = np.arange(g["n"], dtype=np.uint32) if nodes is None else nodes
    rc, lat, loss, _ = O.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], nodes,
                                        rows=rows, threads=4)
    assert rc == 0
    return lat, loss


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _refold_all(g, pred, tl, tf):
    """Every cell's tree path refolds to the table's cell, latency and loss bits."""
    n = g["n"]
    ident = np.arange(n)
    idx = R.build_arc_index(g)
    for s in range(n):
        for d in range(n):
            if s == d:
                continue
            path = R.expand(pred[s], ident, s, d)
            want_lat, want_loss = tl[s].copy(), tf[s].copy()
            lat, loss = R.refold(g, path, want_lat, want_loss, idx)
            assert lat == int(tl[s, d]) and _bits(loss) == _bits(tf[s, d]), (s, d, path)


def test_fold_is_the_oracles_path_add(oracle):
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.random(10000).astype(np.float32), np.float32([0, 1, 0, 1])])
    e = np.concatenate([rng.random(10000).astype(np.float32), np.float32([0, 1, 1, 0])])
    got = R.fold(a, (np.float32(1) - e).astype(np.float32))
    for k in range(len(a)):
        _, want = oracle.path_add(5, float(a[k]), 7, float(e[k]))
        assert _bits(got[k]) == _bits(want), (a[k], e[k])


@pytest.mark.parametrize("directed", [True, False])
def test_reference_graph_trees_refold_to_the_table(oracle, directed):
    """graph/mod.rs:564-651 test_shortest_path."""
    with open(os.path.join(ROOT, "tests", "golden", "reference_kat.json")) as f:
        kat = json.load(f)["test_shortest_path"]
    e = np.array(kat["edges"], np.int64)
    g = dict(n=3, src=e[:, 0].astype(np.uint32), dst=e[:, 1].astype(np.uint32), lat=e[:, 2].astype(np.uint64),
             loss=np.zeros(len(e), np.float32), directed=directed)
    tl, tf = _table(oracle, g)
    assert tl.tolist() == kat["directed_latency" if directed else "undirected_latency"]
    pred, hop, bad = R.tree_ref(g, np.arange(3), (0, 3), tl, tf)
    assert bad is None
    _refold_all(g, pred, tl, tf)
    assert [pred[i, i] for i in range(3)] == [0, 1, 2] and [hop[i, i] for i in range(3)] == [0, 1, 2]
    if directed:
        # 1 -> 2 costs 12 = 1 -> 0 -> 2 (5 + 7); 2 -> 0 costs 16 = 2 -> 1 -> 0 (11 + 5)
        assert pred[1, 2] == 0 and hop[1, 2] == 0 and pred[2, 0] == 1 and hop[2, 0] == 1
        assert pred[0, 1] == 0 and pred[0, 2] == 0 and pred[2, 1] == 2
    else:
        # 1 - 2 costs 10 = 1 - 0 - 2 (3 + 7), below the direct 11
        assert pred[1, 2] == 0 and hop[1, 2] == 0 and pred[2, 1] == 0 and hop[2, 1] == 0
        assert pred[0, 1] == 0 and pred[1, 0] == 1 and pred[0, 2] == 0


def _hand_graph():
    """From node 0: two routes to 3 with equal (latency, loss); two routes to 4 with equal latency,
    one lossless; a parallel pair 3 - 5 of which one arc is lossless; an identical pair 0 - 1."""
    edges = [(0, 1, 0.0), (0, 1, 0.0), (0, 2, 0.0), (1, 3, 0.0), (2, 3, 0.0), (1, 4, 0.1), (2, 4, 0.0), (3, 5, 0.2),
             (3, 5, 0.0)]
    src = list(range(6)) + [a for a, _, _ in edges]
    dst = list(range(6)) + [b for _, b, _ in edges]
    loss = [0.0] * 6 + [f for _, _, f in edges]
    return dict(n=6, src=np.uint32(src), dst=np.uint32(dst), lat=np.full(len(src), 1000, np.uint64),
                loss=np.float32(loss), directed=False)


def test_ties(oracle):
    g = _hand_graph()
    tl, tf = _table(oracle, g)
    pred, hop, bad, cnt = R.tree_ref(g, np.arange(6), (0, 6), tl, tf, counts=True)
    assert bad is None
    # equal (latency, loss) through 1 and through 2: the smaller index wins
    assert cnt[0, 3] == 2 and pred[0, 3] == 1 and hop[0, 3] == 1
    # equal latency, different loss: only the lossless arc 2 -> 4 is tight
    assert tl[0, 4] == 2000 and tf[0, 4] == 0 and cnt[0, 4] == 1 and pred[0, 4] == 2 and hop[0, 4] == 2
    # the parallel pair 3 - 5: each arc counts on its own, and only the lossless one is tight
    assert cnt[0, 5] == 1 and pred[0, 5] == 3 and hop[0, 5] == 1
    # the identical pair 0 - 1: both are tight
    assert cnt[0, 1] == 2 and pred[0, 1] == 0 and hop[0, 1] == 1
    _refold_all(g, pred, tl, tf)
    # the column order does not change the values
    perm = np.array([4, 2, 0, 5, 1, 3], np.uint32)
    pl, pf = _table(oracle, g, perm)
    ppred, phop, pbad = R.tree_ref(g, perm, (0, 6), pl, pf)
    assert pbad is None
    assert np.array_equal(ppred, pred[perm][:, perm]) and np.array_equal(phop, hop[perm][:, perm])


def test_untight_cell_is_reported(oracle):
    g = _hand_graph()
    tl, tf = _table(oracle, g)
    tf = tf.copy()
    tf.view(np.uint32)[2, 5] ^= 1
    pred, _, bad = R.tree_ref(g, np.arange(6), (0, 6), tl, tf)
    assert bad == (2, 5) and pred[2, 5] == 0xFFFFFFFF


def test_suffix_of_a_tree_path_is_not_the_intermediate_nodes_path(oracle):
    """The f32 fold is not associative: walking first hop by first hop across rows leaves the
    source's own path, and its refold misses the table's loss bits."""
    g = TC.suffix_graph()
    n = g["n"]
    tl, tf = _table(oracle, g)
    pred, hop, bad = R.tree_ref(g, np.arange(n), (0, n), tl, tf)
    assert bad is None
    _refold_all(g, pred, tl, tf)
    s, d = TC.SUFFIX_PAIR
    own = R.expand(pred[s], np.arange(n), s, d)
    walk = [s]
    while walk[-1] != d:
        walk.append(int(hop[walk[-1], d]))
    assert own == [6, 0, 3, 2] and walk == [6, 0, 1, 2]
    lat, loss = R.refold(g, walk)
    assert lat == int(tl[s, d]) and _bits(loss) != _bits(tf[s, d])
    lat, loss = R.refold(g, own)
    assert lat == int(tl[s, d]) and _bits(loss) == _bits(tf[s, d])


def _tree_path(pred_row, nodes, src, dst, cap):
    import shadow_amd

    L = shadow_amd.load()
    row = np.ascontiguousarray(pred_row, np.uint32)
    n = len(row)
    nd = None if nodes is None else np.ascontiguousarray(nodes, np.uint32)
    out = np.full(max(cap, 1), 0xDEADBEEF, np.uint32)
    ln = C.c_uint32(0xDEADBEEF)
    rc = L.sg_tree_path(row.ctypes.data, None if nd is None else nd.ctypes.data, n, src, dst, out.ctypes.data, cap,
                        C.byref(ln))
    return rc, out, ln.value


def test_sg_tree_path(oracle):
    from shadow_amd import _capi

    g = _hand_graph()
    tl, tf = _table(oracle, g)
    pred, _, _ = R.tree_ref(g, np.arange(6), (0, 6), tl, tf)
    rc, out, ln = _tree_path(pred[0], None, 0, 5, 6)
    assert rc == _capi.SG_OK and ln == 4 and out[:4].tolist() == [0, 1, 3, 5] and out[4] == 0xDEADBEEF
    # the same row in another column order
    perm = np.array([4, 2, 0, 5, 1, 3], np.uint32)
    rc, out, ln = _tree_path(pred[0][perm], perm, 0, 5, 6)
    assert rc == _capi.SG_OK and out[:ln].tolist() == [0, 1, 3, 5]
    # cap too small: the needed length, nothing written
    rc, out, ln = _tree_path(pred[0], None, 0, 5, 3)
    assert rc == _capi.SG_ERR_CAPACITY and ln == 4 and (out == 0xDEADBEEF).all()
    # src == dst
    rc, out, ln = _tree_path(pred[0], None, 0, 0, 6)
    assert rc == _capi.SG_OK and ln == 1 and out[0] == 0
    # a cyclic row ends; so does one that leaves the range, and a list that is no permutation
    cyc = np.array([0, 2, 1, 1, 2, 3], np.uint32)
    assert _tree_path(cyc, None, 0, 5, 6)[0] == _capi.SG_ERR_INVALID_ARG
    assert _tree_path(np.array([0, 1, 2, 3, 4, 5], np.uint32), None, 0, 5, 6)[0] == _capi.SG_ERR_INVALID_ARG
    assert _tree_path(np.array([0, 0, 0, 99, 0, 3], np.uint32), None, 0, 5, 6)[0] == _capi.SG_ERR_INVALID_ARG
    assert _tree_path(pred[0], np.array([0, 1, 2, 3, 4, 4], np.uint32), 0, 5, 6)[0] == _capi.SG_ERR_INVALID_ARG
    assert _tree_path(pred[0], None, 0, 6, 6)[0] == _capi.SG_ERR_INVALID_ARG


# -- the GPU cases' inputs (test_tree_gpu.py) qualify by the reference alone ------------------
def test_tie_graph_has_ties(oracle):
    """(a): at least 5 % of the cells have two or more tight in-arcs."""
    g = TC.tie_graph()
    assert g["n"] == 300 and not g["directed"]
    assert set((g["lat"] // 1_000_000).tolist()) == {1, 2, 3, 4}
    arc = g["src"] != g["dst"]
    assert 0.55 < (g["loss"][arc] == 0).mean() < 0.65 and 5.5 < 2 * arc.sum() / 300 < 6.5
    tl, tf = _table(oracle, g)
    _, _, bad, cnt = R.tree_ref(g, np.arange(300), (0, 300), tl, tf, counts=True)
    assert bad is None
    frac = (cnt >= 2).mean()
    print(f"tie graph: {frac:.4f} of the cells have two or more tight in-arcs")
    assert frac >= 0.05


def test_wide_graph_rows_mix_wide_and_narrow(oracle):
    """(e): cells at or past 2^32 ns and cells below it in the same row."""
    g = TC.wide_graph()
    tl, tf = _table(oracle, g)
    off = ~np.eye(48, dtype=bool)
    wide = (tl >= TC.WIDE_NS) & off
    narrow = (tl < TC.WIDE_NS) & off
    assert (wide.any(1) & narrow.any(1)).all()
    assert R.tree_ref(g, np.arange(48), (0, 48), tl, tf)[2] is None
