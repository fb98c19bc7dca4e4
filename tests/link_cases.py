"""Graphs and traffic matrices of the link-load tests (test_link_ref_cpu.py qualifies them on the
CPU, test_link_gpu.py runs them).  The graphs of tests/tree_cases.py are reused by import."""
import numpy as np

from tree_cases import c3_graph, directed_graph, multi_graph, sparse_graph, tie_graph  # noqa: F401

SENT64 = np.uint64(0xA5A5A5A500000000)  # the outputs start from this: "adds into" is itself checked
ZERO_ROWS = (3, 17, 18, 19, 64, 100, 150, 222, 298, 299)  # (b)'s all-zero rows


def _graph(n, src, dst, lat, directed=False):
    m = len(src)
    return dict(n=n, src=np.asarray(src, np.uint32), dst=np.asarray(dst, np.uint32), lat=np.asarray(lat, np.uint64),
                loss=np.zeros(m, np.float32), directed=directed)


def path_graph(n=4096):
    """(f): 0 - 1 - ... - n-1 with a self-loop per node: a tree of depth n - 1 from either end."""
    v = np.arange(n)
    src = np.concatenate([v, v[:-1]])
    dst = np.concatenate([v, v[1:]])
    return _graph(n, src, dst, np.full(len(src), 1_000_000))


def star_graph(spokes=512):
    """(f): node 0 joined to `spokes` nodes by 1 ms arcs, the spokes in a ring of 5 ms arcs: from a
    spoke, every other node but its two ring neighbours is reached through the hub."""
    n = spokes + 1
    v = np.arange(n)
    sp = np.arange(1, n)
    src = np.concatenate([v, np.zeros(spokes, np.int64), sp])
    dst = np.concatenate([v, sp, np.where(sp == spokes, 1, sp + 1)])
    lat = np.concatenate([np.full(n, 1_000_000), np.full(spokes, 1_000_000), np.full(spokes, 5_000_000)])
    return _graph(n, src, dst, lat)


def dense_matrix(rows, cols, seed=11):
    """(a): every cell in 1 .. 1000, the diagonal included."""
    return np.random.default_rng(seed).integers(1, 1001, (rows, cols)).astype(np.uint64)


def sparse_matrix(rows=300, cols=300, seed=12):
    """(b): 2 % of the cells nonzero, values up to 2^40, the rows of ZERO_ROWS all zero."""
    rng = np.random.default_rng(seed)
    c = np.where(rng.random((rows, cols)) < 0.02, rng.integers(1, 1 << 40, (rows, cols)), 0).astype(np.uint64)
    c[list(ZERO_ROWS)] = 0
    return c


def packet_matrix(rows, cols, packets, seed=13):
    """(h): `packets` packets on uniform random pairs, as an np.add.at matrix."""
    rng = np.random.default_rng(seed)
    c = np.zeros((rows, cols), np.uint64)
    np.add.at(c, (rng.integers(0, rows, packets), rng.integers(0, cols, packets)), np.uint64(1))
    return c


def tree_shape(pred_row, nodes, s):
    """(depth, largest fan-out, leaves) of one pred row."""
    n = len(pred_row)
    par = np.empty(n, np.int64)
    par[np.asarray(nodes, np.int64)] = np.asarray(pred_row, np.int64)
    kids = np.bincount(par[np.arange(n) != s], minlength=n)
    depth = np.zeros(n, np.int64)
    cur = np.arange(n)
    for d in range(1, n + 1):
        live = cur != s
        if not live.any():
            break
        depth[live] = d
        cur = np.where(live, par[cur], s)
    return int(depth.max()), int(kids.max()), int((kids == 0).sum())
