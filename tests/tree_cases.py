"""Graphs of the shortest-path tree tests (test_tree_ref_cpu.py qualifies them on the CPU,
test_tree_gpu.py runs them)."""
import numpy as np

from shadow_amd import synth

TIE_SEED = 5
WIDE_SEED = 3
WIDE_NS = 1 << 32


def _graph(n, src, dst, lat, loss, directed):
    return dict(n=n, src=np.asarray(src, np.uint32), dst=np.asarray(dst, np.uint32), lat=np.asarray(lat, np.uint64),
                loss=np.asarray(loss, np.float32), directed=directed)


def tie_graph(n=300, seed=TIE_SEED):
    """(a): undirected, mean degree 6, latencies from {1, 2, 3, 4} ms, 60 % zero-loss arcs: many
    cells have several optimal routes."""
    rng = np.random.default_rng(seed)
    ring = np.arange(n)
    k = 3 * n - n
    cs, cd = rng.integers(0, n, k), rng.integers(0, n, k)
    keep = cs != cd
    src = np.concatenate([ring, ring, cs[keep]])
    dst = np.concatenate([ring, (ring + 1) % n, cd[keep]])
    m = len(src)
    lat = rng.integers(1, 5, m).astype(np.uint64) * 1_000_000
    # the lossy arcs: one in ten uniform (their folds round), the rest 0.5 (their folds are exact,
    # so routes through equally many of them tie bit for bit, as zero-loss routes do)
    loss = rng.uniform(0.0, 0.02, m).astype(np.float32)
    loss[rng.random(m) < 0.9] = 0.5
    loss[rng.random(m) < 0.6] = 0.0
    return _graph(n, src, dst, lat, loss, False)


def directed_graph(seed=5):
    """(c): 257 nodes, a ring (both ways, weights of their own) plus random arcs."""
    return synth.ring_chords_graph(257, 6.0, seed=seed, directed=True)


def multi_graph(seed=7):
    """(d): 64 nodes with parallel edges and self-loops."""
    return synth.ring_chords_graph(64, 6.0, seed=seed, parallel=0.3)


def wide_graph(seed=WIDE_SEED):
    """(e): a 48-node ring with 1-3 s arcs: paths of 2^32 ns and more beside shorter ones."""
    return synth.ring_chords_graph(48, 2.0, seed=seed, lat_lo_us=1_000_000, lat_hi_us=3_000_000)


def sparse_graph(n, seed=9):
    """(g): mean degree 4."""
    return synth.ring_chords_graph(n, 4.0, seed=seed)


def c3_graph():
    """(h): the C3 shape, 10,000 nodes at mean degree 8."""
    return synth.ring_chords_graph(10000, 8.0, seed=1)


SUFFIX_SEED, SUFFIX_PAIR = 1816, (6, 2)


def suffix_graph(n=7, seed=SUFFIX_SEED):
    """Seven nodes, every arc 1 us, losses from four values: many equal-latency routes whose f32
    folds differ in the last bits with the order of the factors.  Seed found by a CPU search:
    for SUFFIX_PAIR the row's own path and the first-hop-by-first-hop walk across rows differ."""
    rng = np.random.default_rng(seed)
    m = 2 * n
    cs, cd = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = cs != cd
    ring = np.arange(n)
    src = np.concatenate([ring, ring, cs[keep]])
    dst = np.concatenate([ring, (ring + 1) % n, cd[keep]])
    mm = len(src)
    lat = np.full(mm, 1000, np.uint64)
    loss = rng.choice(np.array([0.1, 0.2, 0.3, 0.05], np.float32), mm)
    return _graph(n, src, dst, lat, loss, False)


def hub_graph(n=513, seed=13):
    """(i): a ring plus node 0 joined to every other node: in-degree 512."""
    rng = np.random.default_rng(seed)
    ring = np.arange(n)
    spokes = np.arange(2, n - 1)  # (1 and n - 1 are the hub's ring neighbours)
    src = np.concatenate([ring, ring, np.zeros(len(spokes), np.int64)])
    dst = np.concatenate([ring, (ring + 1) % n, spokes])
    m = len(src)
    lat = rng.integers(1, 40, m).astype(np.uint64) * 1_000_000
    loss = rng.uniform(0.0, 0.02, m).astype(np.float32)
    loss[rng.random(m) < 0.5] = 0.0
    return _graph(n, src, dst, lat, loss, False)
