"""The graphs of test_sssp_plan_gpu.py, shared with test_plan_ref_cpu.py, which pins the
properties of their plans that the GPU tests rely on."""
import numpy as np

from shadow_amd import synth


def ties(g, seed, zero=0.6):
    """test_sssp_chain_gpu's family: latencies of 1-4 us in 1 us steps (equal-latency paths), a
    share `zero` of zero-loss arcs."""
    rng = np.random.default_rng(seed)
    g["lat"] = (rng.integers(1, 5, len(g["lat"])) * 1000).astype(np.uint64)
    loss = rng.uniform(0.01, 0.3, len(g["lat"])).astype(np.float32)
    loss[rng.random(len(loss)) < zero] = 0
    g["loss"] = loss
    return g


def _add_edges(g, src, dst):
    g["src"] = np.concatenate([g["src"], np.asarray(src, dtype=np.uint32)])
    g["dst"] = np.concatenate([g["dst"], np.asarray(dst, dtype=np.uint32)])
    g["lat"] = np.concatenate([g["lat"], np.zeros(len(src), dtype=np.uint64)])
    g["loss"] = np.concatenate([g["loss"], np.zeros(len(src), dtype=np.float32)])
    return g


def big():
    """2,400 nodes: every phase of a 3- or 4-phase plan holds more rows than the grid has
    persistent workgroups (256), so rows chain inside bounded launches."""
    return ties(synth.ring_chords_graph(2400, 7.0, seed=31), 31)


def small():
    """test_chains_form's 900 nodes: at 6 phases the late phases are smaller than the grid."""
    return ties(synth.ring_chords_graph(900, 7.0, seed=31), 31)


def star(zero=0.6):
    """600 nodes, each with a self-loop; node 0 has an edge to every other (out-degree 599)."""
    n = 600
    g = dict(n=n, src=np.arange(n, dtype=np.uint32), dst=np.arange(n, dtype=np.uint32),
             lat=np.zeros(n, dtype=np.uint64), loss=np.zeros(n, dtype=np.float32), directed=False)
    _add_edges(g, np.zeros(n - 1), np.arange(1, n))
    return ties(g, 600, zero)


def hubs(zero=0.6):
    """800 nodes with parallel edges, a 150-spoke hub (node 0), a 40-spoke hub (node 400) and six
    nodes given 6-16 more edges: out-degrees on both sides of 8 (the lane path's arcs per lane) and
    of 64 (SG_SSSP_LANE_DEG's default, the chain scan's cap)."""
    g = synth.ring_chords_graph(800, 7.0, seed=44, parallel=0.3)
    rng = np.random.default_rng(44)
    others = lambda v, k: rng.permutation(np.setdiff1d(np.arange(800), [v]))[:k]
    _add_edges(g, np.zeros(150), others(0, 150))
    _add_edges(g, np.full(40, 400), others(400, 40))
    for v, k in ((100, 6), (200, 8), (300, 10), (500, 12), (600, 14), (700, 16)):
        _add_edges(g, np.full(k, v), others(v, k))
    return ties(g, 44, zero)


def far():
    """test_chain_behind_saturated_rows' 620 nodes: every arc of each 23rd node is 5 s long, past
    the 32-bit keys (LAT32_SAT), so with every node used each row holds saturated keys and the
    wide kernel finishes the table."""
    n = 620
    g = ties(synth.ring_chords_graph(n, 6.0, seed=22), 22)
    far_nodes = np.arange(0, n, 23)
    sel = (np.isin(g["src"], far_nodes) | np.isin(g["dst"], far_nodes)) & (g["src"] != g["dst"])
    g["lat"][sel] = np.uint64(5_000_000_000)
    return g


def directed():
    return ties(synth.ring_chords_graph(700, 7.0, seed=9, directed=True), 9)


def out_degrees(g):
    s, d = g["src"].astype(np.int64), g["dst"].astype(np.int64)
    keep = s != d
    s, d = s[keep], d[keep]
    if not g["directed"]:
        s = np.concatenate([s, d])
    return np.bincount(s, minlength=g["n"])


SUBSET = np.random.default_rng(1801).permutation(2400)[:1801].astype(np.uint32)  # of big(), shuffled
