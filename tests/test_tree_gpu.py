"""Shortest-path trees on the GPU (sg_routing_tree, sg_routing_build_tree, PathTree).

Every case first asserts that the library's rows equal the oracle's, then compares pred and
first_hop bit for bit with tests/tree_ref.py on the oracle's rows, then refolds 200 sampled tree
paths to the table's bits.  The inputs' own conditions (ties in (a), wide and narrow cells in one
row of (e)) are checked on the CPU in test_tree_ref_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import tree_cases as TC
import tree_ref as R

pytestmark = pytest.mark.gpu

SENT32 = 0xA5A5A5A5


def _graph_net(g, ctx):
    from shadow_amd import NetworkGraph

    return NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)


def _oracle_rows(O, g, nodes, r0, r1):
    rc, lat, loss, _ = O.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"],
                                        np.asarray(nodes, np.uint32), rows=(r0, r1), threads=8)
    assert rc == 0
    return lat, loss


def _build_tree(net, nodes, r0, r1):
    """sg_routing_build_tree with host outputs: (lat, loss, pred, first_hop)."""
    from shadow_amd import _capi

    nodes = np.ascontiguousarray(nodes, np.uint32)
    n, k = len(nodes), r1 - r0
    lat, loss = np.zeros((k, n), np.uint64), np.zeros((k, n), np.float32)
    pred, hop = np.full((k, n), SENT32, np.uint32), np.full((k, n), SENT32, np.uint32)
    _capi.check(net.ctx.handle, _capi.load().sg_routing_build_tree(
        net.ctx.handle, net._ensure_net(), nodes.ctypes.data, n, r0, r1, _capi.SG_ROUTE_SHORTEST_PATH,
        lat.ctypes.data, loss.ctypes.data, pred.ctypes.data, hop.ctypes.data))
    return lat, loss, pred, hop


def _check(O, g, nodes, r0, r1, got, seed=1, want=None):
    """The three steps of every case; returns the reference (pred, first_hop)."""
    nodes = np.asarray(nodes, np.uint32)
    lat, loss, pred, hop = got
    olat, oloss = want[:2] if want else _oracle_rows(O, g, nodes, r0, r1)
    assert np.array_equal(lat, olat), "latency rows differ from the oracle's"
    assert np.array_equal(loss.view(np.uint32), oloss.view(np.uint32)), "loss rows differ from the oracle's"
    rpred, rhop, bad = want[2:] if want else R.tree_ref(g, nodes, (r0, r1), olat, oloss)
    assert bad is None
    assert np.array_equal(pred, rpred), f"pred differs in {int((pred != rpred).sum())} cells"
    assert np.array_equal(hop, rhop), f"first_hop differs in {int((hop != rhop).sum())} cells"
    rng = np.random.default_rng(seed)
    idx = R.build_arc_index(g)
    n = g["n"]
    for i, j in zip(rng.integers(0, r1 - r0, 200).tolist(), rng.integers(0, n, 200).tolist()):
        s, d = int(nodes[r0 + i]), int(nodes[j])
        if s == d:
            continue
        path = R.expand(pred[i], nodes, s, d)
        assert path[1] == hop[i, j]
        wl, wf = np.zeros(n, np.uint64), np.zeros(n, np.float32)
        wl[nodes], wf[nodes] = olat[i], oloss[i]
        l2, f2 = R.refold(g, path, wl, wf, idx)
        assert l2 == int(olat[i, j]) and np.float32(f2).view(np.uint32) == oloss[i, j].view(np.uint32), (s, d, path)
    return rpred, rhop


@pytest.fixture(scope="module")
def tie(oracle):
    """(a)'s graph, the oracle's table and the reference trees, computed once."""
    g = TC.tie_graph()
    nodes = np.arange(g["n"], dtype=np.uint32)
    olat, oloss = _oracle_rows(oracle, g, nodes, 0, g["n"])
    rpred, rhop, bad = R.tree_ref(g, nodes, (0, g["n"]), olat, oloss)
    return dict(g=g, nodes=nodes, want=(olat, oloss, rpred, rhop, bad))


@pytest.fixture(scope="module")
def directed(oracle):
    g = TC.directed_graph()
    nodes = np.arange(g["n"], dtype=np.uint32)
    olat, oloss = _oracle_rows(oracle, g, nodes, 0, g["n"])
    rpred, rhop, bad = R.tree_ref(g, nodes, (0, g["n"]), olat, oloss)
    return dict(g=g, nodes=nodes, want=(olat, oloss, rpred, rhop, bad))


def _lds_rows(ctx):
    """(rows the last tree pass launched on the LDS path, the LDS path's node limit); timers on."""
    _, rows, n_max = ctx.read_timer("tree_lds")
    return int(rows), int(n_max)


def test_ties_lds_path(oracle, ctx, tie):
    """(a)"""
    g = tie["g"]
    net = _graph_net(g, ctx)
    ctx.enable_timers(True)
    try:
        got = _build_tree(net, tie["nodes"], 0, g["n"])
        assert _lds_rows(ctx)[0] == g["n"]
        assert ctx.read_timer("tree")[1] == 1
    finally:
        ctx.enable_timers(False)
    _check(oracle, g, tie["nodes"], 0, g["n"], got, want=tie["want"])


def test_permutation_and_row_block(oracle, ctx, tie):
    """(b): the outputs are petgraph indices, so a shuffled column order only re-indexes them."""
    g = tie["g"]
    nodes = np.random.default_rng(4).permutation(g["n"]).astype(np.uint32)
    got = _build_tree(_graph_net(g, ctx), nodes, 37, 201)
    _check(oracle, g, nodes, 37, 201, got)
    rpred, rhop = tie["want"][2:4]
    assert np.array_equal(got[2], rpred[nodes[37:201]][:, nodes])
    assert np.array_equal(got[3], rhop[nodes[37:201]][:, nodes])


def test_directed(oracle, ctx, directed):
    """(c)"""
    g = directed["g"]
    got = _build_tree(_graph_net(g, ctx), directed["nodes"], 0, g["n"])
    _check(oracle, g, directed["nodes"], 0, g["n"], got, want=directed["want"])


def test_multigraph(oracle, ctx):
    """(d)"""
    g = TC.multi_graph()
    keep = g["src"] != g["dst"]
    pairs = np.stack([np.minimum(g["src"], g["dst"])[keep], np.maximum(g["src"], g["dst"])[keep]], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs) and (~keep).sum() == 64  # parallel edges, self-loops
    nodes = np.arange(64, dtype=np.uint32)
    _check(oracle, g, nodes, 0, 64, _build_tree(_graph_net(g, ctx), nodes, 0, 64))


def test_wide_rows_take_the_global_path(oracle, ctx):
    """(e): rows holding latencies of 2^32 ns and more leave the LDS kernel by themselves."""
    g = TC.wide_graph()
    nodes = np.arange(48, dtype=np.uint32)
    got = _build_tree(_graph_net(g, ctx), nodes, 0, 48)
    assert (got[0] >= TC.WIDE_NS).any()
    _check(oracle, g, nodes, 0, 48, got)


@pytest.mark.parametrize("which", ["tie", "directed"])
def test_forced_global_path(oracle, ctx, tie, directed, which, monkeypatch):
    """(f): SG_TREE_LDS=0 gives the LDS path's outputs."""
    case = tie if which == "tie" else directed
    g = case["g"]
    net = _graph_net(g, ctx)
    lds = _build_tree(net, case["nodes"], 0, g["n"])
    monkeypatch.setenv("SG_TREE_LDS", "0")
    ctx.enable_timers(True)
    try:
        glob = _build_tree(net, case["nodes"], 0, g["n"])
        assert _lds_rows(ctx)[0] == 0
    finally:
        ctx.enable_timers(False)
    _check(oracle, g, case["nodes"], 0, g["n"], glob, want=case["want"])
    assert np.array_equal(lds[2], glob[2]) and np.array_equal(lds[3], glob[3])


def test_lds_limit(oracle, ctx):
    """(g): the largest n the LDS path takes (from the device's LDS size), and n + 1."""
    ctx.enable_timers(True)
    try:
        g0 = TC.sparse_graph(64)
        _build_tree(_graph_net(g0, ctx), np.arange(64, dtype=np.uint32), 0, 8)
        n_max = _lds_rows(ctx)[1]
        assert 4096 <= n_max < 65535
        for n, lds_rows in ((n_max, 64), (n_max + 1, 0)):
            g = TC.sparse_graph(n)
            nodes = np.arange(n, dtype=np.uint32)
            r0 = n // 2 - 32
            got = _build_tree(_graph_net(g, ctx), nodes, r0, r0 + 64)
            assert _lds_rows(ctx)[0] == lds_rows, n
            _check(oracle, g, nodes, r0, r0 + 64, got)
    finally:
        ctx.enable_timers(False)


def test_c3_shape(oracle, ctx):
    """(h): rows [4872, 5128) of a 10,000-node C3-style graph: the 80-KB key layout."""
    g = TC.c3_graph()
    nodes = np.arange(10000, dtype=np.uint32)
    _check(oracle, g, nodes, 4872, 5128, _build_tree(_graph_net(g, ctx), nodes, 4872, 5128))


def test_hub(oracle, ctx):
    """(i): a node of in-degree 512 is walked by its wave, not by one lane."""
    g = TC.hub_graph()
    deg = np.bincount(np.concatenate([g["src"], g["dst"]])[np.tile(g["src"] != g["dst"], 2)], minlength=513)
    assert deg[0] == 512
    nodes = np.arange(513, dtype=np.uint32)
    _check(oracle, g, nodes, 0, 513, _build_tree(_graph_net(g, ctx), nodes, 0, 513))


def test_used_subset(oracle, ctx, tie):
    """(j): 40 used nodes placed first, rows [0, 40); the leading 40 columns are the ordinary
    build's table over the used nodes."""
    g = tie["g"]
    used = np.random.default_rng(8).choice(300, 40, replace=False).astype(np.uint32)
    net = _graph_net(g, ctx)
    t = net.compute_shortest_path_tree(used)
    assert np.array_equal(t.nodes[:40], used) and sorted(t.nodes.tolist()) == list(range(300))
    _check(oracle, g, t.nodes, 0, 40, (t.latency_ns, t.packet_loss, t.pred, t.first_hop))
    tab = net.compute_shortest_paths(used)
    # (the diagonal holds the self-loop in both)
    assert np.array_equal(t.latency_ns[:, :40], tab.latency_ns)
    assert np.array_equal(t.packet_loss[:, :40].view(np.uint32), tab.packet_loss.view(np.uint32))


def test_corrupted_table(oracle, ctx, tie):
    """(k): one loss bit flipped in a device row: SG_ERR_INVALID_ARG naming the first untight cell."""
    import torch

    from shadow_amd import ShadowGpuError, _capi

    g, nodes = tie["g"], tie["nodes"]
    n = g["n"]
    net = _graph_net(g, ctx)
    dlat = torch.zeros((n, n), dtype=torch.int64, device="cuda")
    dloss = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    dpred = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    dhop = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    net.build_rows_device(nodes, 0, n, dlat.data_ptr(), dloss.data_ptr())
    net.tree_rows_device(nodes, 0, n, dlat.data_ptr(), dloss.data_ptr(), dpred.data_ptr(), dhop.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(dpred.cpu().numpy().view(np.uint32), tie["want"][2])
    assert np.array_equal(dhop.cpu().numpy().view(np.uint32), tie["want"][3])
    # either output alone
    net.tree_rows_device(nodes, 0, n, dlat.data_ptr(), dloss.data_ptr(), 0, dhop.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(dhop.cpu().numpy().view(np.uint32), tie["want"][3])
    olat, oloss = tie["want"][0], tie["want"][1].copy()
    assert olat[17, 123] > 0
    oloss.view(np.uint32)[17, 123] ^= 1
    first = R.tree_ref(g, nodes, (0, n), olat, oloss)[2]
    assert first is not None and first[0] == 17
    bits = dloss.view(torch.int32)
    bits[17, 123] ^= 1
    torch.cuda.synchronize()
    with pytest.raises(ShadowGpuError) as e:
        net.tree_rows_device(nodes, 0, n, dlat.data_ptr(), dloss.data_ptr(), dpred.data_ptr(), dhop.data_ptr())
    assert e.value.code == _capi.SG_ERR_INVALID_ARG and e.value.pair == first
    assert "tight" in str(e.value)


def test_argument_errors(ctx, tie):
    """(l): SG_ERR_INVALID_ARG, the output buffers still holding their sentinel."""
    from shadow_amd import _capi

    g = tie["g"]
    n = g["n"]
    net = _graph_net(g, ctx)
    L, h, nh = _capi.load(), ctx.handle, net._ensure_net()
    nodes = np.arange(n, dtype=np.uint32)
    lat, loss = np.full((4, n), 0x5A5A5A5A5A5A5A5A, np.uint64), np.full((4, n), -7.0, np.float32)
    pred, hop = np.full((4, n), SENT32, np.uint32), np.full((4, n), SENT32, np.uint32)
    SP = _capi.SG_ROUTE_SHORTEST_PATH

    def tree(nd, k, r0, r1, p=pred.ctypes.data, f=hop.ctypes.data):
        return L.sg_routing_tree(h, nh, nd.ctypes.data, k, r0, r1, 0, lat.ctypes.data, loss.ctypes.data, p, f)

    def build_tree(nd, k, r0, r1, flags, p=pred.ctypes.data):
        return L.sg_routing_build_tree(h, nh, nd.ctypes.data, k, r0, r1, flags, lat.ctypes.data, loss.ctypes.data,
                                       p, hop.ctypes.data)

    dup = nodes.copy()
    dup[5] = 6
    out = nodes.copy()
    out[9] = n
    bad = [tree(dup, n, 0, 4), tree(out, n, 0, 4), tree(nodes[:40], 40, 0, 4), tree(nodes, n, 0, 4, None, None),
           tree(nodes, n, 3, 2), tree(nodes, n, n - 1, n + 1),
           build_tree(dup, n, 0, 4, SP), build_tree(nodes, n, 0, 4, 0), build_tree(nodes, n, 2, n + 1, SP),
           build_tree(nodes, n, 0, 4, SP, None)]
    assert bad == [_capi.SG_ERR_INVALID_ARG] * len(bad)
    assert (pred == SENT32).all() and (hop == SENT32).all()
    assert (lat == 0x5A5A5A5A5A5A5A5A).all() and (loss == -7.0).all()
    # and the context still works
    assert build_tree(nodes, n, 0, 4, SP) == _capi.SG_OK
    assert np.array_equal(pred, tie["want"][2][:4]) and np.array_equal(hop, tie["want"][3][:4])


def test_python_path_tree(oracle, ctx, tie):
    """(m): PathTree.path / .path_properties."""
    from shadow_amd import PathTree

    g = tie["g"]
    net = _graph_net(g, ctx)
    t = net.compute_shortest_path_tree()
    assert isinstance(t, PathTree) and t.n_sources == 300
    olat, oloss, rpred = tie["want"][:3]
    assert np.array_equal(t.pred, rpred)
    rng = np.random.default_rng(3)
    for s, d in zip(rng.integers(0, 300, 60).tolist(), rng.integers(0, 300, 60).tolist()):
        path = t.path(s, d)
        assert path == R.expand(rpred[s], tie["nodes"], s, d)
        p = t.path_properties(s, d)
        if s == d:
            assert path == [s] and p.latency_ns == 0 and p.packet_loss == 0
        else:
            assert p.latency_ns == int(olat[s, d])
            assert np.float32(p.packet_loss).view(np.uint32) == oloss[s, d].view(np.uint32)
    sub = net.compute_shortest_path_tree([7, 3])
    assert sub.path(3, 250) == t.path(3, 250)
    with pytest.raises(KeyError):
        sub.path(250, 3)
