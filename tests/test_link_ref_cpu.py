"""The link-load reference (tests/link_ref.py) on a hand graph with the expected loads written
out, its conservation laws, and the conditions the GPU cases' inputs must meet
(test_link_gpu.py), checked here so that the inputs qualify by the references alone.  No GPU."""
import numpy as np

import link_cases as LC
import link_ref as LR
import tree_ref as R


def _trees(O, g, nodes=None, rows=None):
    """pred rows (tests/tree_ref.py) from the oracle's table."""
    nodes = np.arange(g["n"], dtype=np.uint32) if nodes is None else nodes
    rows = (0, g["n"]) if rows is None else rows
    rc, lat, loss, _ = O.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], nodes,
                                        rows=rows, threads=4)
    assert rc == 0
    pred, _, bad = R.tree_ref(g, nodes, rows, lat, loss)
    assert bad is None
    return pred


def _hand_graph():
    """A tree plus one chord and a parallel pair, 1 us arcs except the chord:
           0 - 1 - 3        1 = 1 (two edges)     4 - 5 costs 9 us (never on a shortest path)
           |   |
           2   4            2 - 5
    """
    edges = [(0, 1, 1), (0, 1, 1), (0, 2, 1), (1, 3, 1), (1, 4, 1), (2, 5, 1), (4, 5, 9)]
    src = list(range(6)) + [a for a, _, _ in edges]
    dst = list(range(6)) + [b for _, b, _ in edges]
    lat = [1000] * 6 + [1000 * w for _, _, w in edges]
    return dict(n=6, src=np.uint32(src), dst=np.uint32(dst), lat=np.uint64(lat), loss=np.zeros(len(src), np.float32),
                directed=False)


def test_hand_graph(oracle):
    g = _hand_graph()
    tail, head, keys = LR.links(g)
    # 6 self-loops and 2 x 6 distinct pairs; ascending (head, tail)
    assert len(keys) == 18
    assert list(zip(tail.tolist(), head.tolist()))[:4] == [(0, 0), (1, 0), (2, 0), (0, 1)]
    fwd, rev = LR.edge_links(g)
    assert fwd[6] == fwd[7] and rev[6] == rev[7] and fwd[6] != rev[6]  # the parallel pair shares its links
    assert np.array_equal(fwd[:6], rev[:6])  # a self-loop names one link
    pred = _trees(oracle, g)
    assert pred[0].tolist() == [0, 0, 0, 1, 1, 2]
    # row 0 sends 1, 2, 4, 8, 16 to nodes 1 .. 5 and 7 to itself; row 3 sends 100 to node 5
    c = np.zeros((6, 6), np.uint64)
    c[0] = [7, 1, 2, 4, 8, 16]
    c[3, 5] = 100
    link, node = LR.link_load(g, np.arange(6), (0, 6), pred, c)
    k = lambda u, v: int(LR.link_index(keys, [u], [v])[0])
    want = np.zeros(18, np.uint64)
    want[k(0, 0)] = 7
    want[k(0, 1)] = 1 + 4 + 8
    want[k(0, 2)] = 2 + 16 + 100  # row 3's path is 3 - 1 - 0 - 2 - 5
    want[k(1, 3)] = 4
    want[k(1, 4)] = 8
    want[k(2, 5)] = 16 + 100
    want[k(3, 1)] = 100
    want[k(1, 0)] = 100  # (3 - 1 - 0 crosses (1, 0), not (0, 1))
    assert np.array_equal(link, want)
    assert node.tolist() == [100, 13 + 100, 18 + 100, 4, 8, 16 + 100]
    # a column subset and a shuffled order give the same loads
    perm = np.array([3, 0, 5, 1, 2, 4], np.uint32)
    ppred = _trees(oracle, g, perm)
    pc = c[perm][:, perm]
    l2, n2 = LR.link_load(g, perm, (0, 6), ppred, pc)
    assert np.array_equal(l2, link) and np.array_equal(n2, node)
    # two row blocks add up
    l3, n3 = LR.link_load(g, perm, (0, 2), ppred[:2], pc[:2])
    l3, n3 = LR.link_load(g, perm, (2, 6), ppred[2:], pc[2:], l3, n3)
    assert np.array_equal(l3, link) and np.array_equal(n3, node)


def test_conservation_on_tie_graph(oracle):
    g = LC.tie_graph()
    n = g["n"]
    nodes = np.arange(n, dtype=np.uint32)
    pred = _trees(oracle, g)
    c = LC.dense_matrix(n, n)
    tail, head, _ = LR.links(g)
    hops = np.zeros((n, n), np.int64)
    rng = np.random.default_rng(2)
    rows = rng.choice(n, 12, replace=False)
    total = 0
    for i in rows.tolist():
        link, node = LR.link_load(g, nodes, (i, i + 1), pred[i:i + 1], c[i:i + 1])
        off = int(c[i].sum() - c[i, i])
        # everything the source sends leaves it over its own links
        assert int(link[(tail == i) & (head != i)].sum()) == off
        assert int(link[(tail == i) & (head == i)].sum()) == int(c[i, i])
        for j in range(n):
            hops[i, j] = len(R.expand(pred[i], nodes, i, j)) - 1
        assert int(link[tail != head].sum()) == int((c[i].astype(np.int64) * hops[i]).sum())
        assert int(node.sum()) == int(link[tail != head].sum()) and node[i] == 0
        total += 1
    assert total == 12


def test_gpu_inputs_qualify(oracle):
    """(a) and (d): deep and wide enough trees; (e): fewer links than ordered edge endpoints."""
    for g in (LC.tie_graph(), LC.directed_graph()):
        pred = _trees(oracle, g, rows=(0, 1))
        depth, fan, leaves = LC.tree_shape(pred[0], np.arange(g["n"]), 0)
        print(f"n={g['n']} row 0: depth {depth}, largest fan-out {fan}, {leaves} leaves")
        assert depth >= 5 and fan >= 4
    g = LC.directed_graph()
    tail, head, keys = LR.links(g)
    both = set(zip(tail.tolist(), head.tolist()))
    assert any((v, u) not in both for u, v in both if u != v)  # some pair has one direction only
    g = LC.multi_graph()
    _, _, keys = LR.links(g)
    loops = int((g["src"] == g["dst"]).sum())
    endpoints = 2 * (len(g["src"]) - loops) + loops
    print(f"multi_graph: {len(g['src'])} edges, {loops} self-loops, {len(keys)} links, {endpoints} ordered endpoints")
    assert loops == 64 and len(keys) < endpoints
    fwd, rev = LR.edge_links(g)
    assert len(np.unique(fwd)) < len(fwd)  # parallel edges share a link


def test_shape_extremes_qualify(oracle):
    """(f): the path graph's depth and the star's hub; (h): the C3 shape."""
    g = LC.path_graph(4096)
    pred = _trees(oracle, g, rows=(0, 1))
    assert LC.tree_shape(pred[0], np.arange(4096), 0)[0] == 4095
    pred = _trees(oracle, g, rows=(2048, 2049))
    assert LC.tree_shape(pred[0], np.arange(4096), 2048) == (2048, 2, 2)
    g = LC.star_graph()
    pred = _trees(oracle, g, rows=(1, 2))
    depth, fan, leaves = LC.tree_shape(pred[0], np.arange(513), 1)
    assert depth == 2 and fan >= 500 and int((pred[0] == 0).sum()) == fan  # the hub's children
    g = LC.c3_graph()
    pred = _trees(oracle, g, rows=(0, 1))
    depth, fan, leaves = LC.tree_shape(pred[0], np.arange(10000), 0)
    print(f"C3 row 0: depth {depth}, largest fan-out {fan}, {leaves} leaves")
    assert depth >= 5 and 3000 <= leaves <= 7000


def test_sparse_matrix_qualifies(oracle):
    """(b): all-zero rows, and subtree sums of 2^32 and more."""
    g = LC.tie_graph()
    c = LC.sparse_matrix()
    assert sum(1 for i in range(300) if not c[i].any()) >= 10 and int(c.max()) < 1 << 40
    nz = (c != 0).mean()
    assert 0.015 < nz < 0.025
    pred = _trees(oracle, g, rows=(0, 1))
    _, node = LR.link_load(g, np.arange(300), (0, 1), pred, c[:1])
    assert int(node.max()) >= 1 << 32


def test_first_bad(oracle):
    """The corrupted rows of (j), by the reference's own rules."""
    g = LC.tie_graph()
    n = g["n"]
    nodes = np.arange(n, dtype=np.uint32)
    pred = _trees(oracle, g, rows=(0, 16))
    c = LC.dense_matrix(16, n)
    assert LR.first_bad(g, nodes, (0, 16), pred, c) is None
    p = pred.copy()
    a = 40
    b = int(p[7, a])
    assert b != 7
    p[7, b] = a  # a 2-cycle a <-> b
    assert LR.first_bad(g, nodes, (0, 16), p, c) == (7, min(a, b))
    p = pred.copy()
    p[5, 123] = n
    assert LR.first_bad(g, nodes, (0, 16), p, c) == (5, 123)
    p = pred.copy()
    p[9, 9] = 10
    assert LR.first_bad(g, nodes, (0, 16), p, c) == (9, 9)
    c0 = c.copy()
    c0[9] = 0
    assert LR.first_bad(g, nodes, (0, 16), p, c0) is None  # an all-zero row is not validated
