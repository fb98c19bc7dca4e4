"""Link loads on the GPU (sg_net_links, sg_net_edge_links, sg_link_load, PathTree.link_load).

In every case the pred rows come from sg_routing_build_tree on the same net: their own
correctness is test_tree_gpu.py's, here they are inputs.  The outputs start from a nonzero
sentinel pattern, so that "adds into" is itself checked, and every comparison with
tests/link_ref.py is exact (np.array_equal on u64).  The inputs' own conditions (deep and wide
trees, parallel edges, all-zero rows, sums past 2^32) are checked on the CPU in
test_link_ref_cpu.py."""
import numpy as np
import pytest

import link_cases as LC
import link_ref as LR

pytestmark = pytest.mark.gpu

SENT = LC.SENT64
UMAX = 0xFFFFFFFF


def _net(g, ctx):
    from shadow_amd import NetworkGraph

    return NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)


def _pred(net, nodes, r0, r1):
    """pred rows [r0, r1) from sg_routing_build_tree (host outputs)."""
    from shadow_amd import _capi

    nodes = np.ascontiguousarray(nodes, np.uint32)
    n, k = len(nodes), r1 - r0
    lat, loss = np.zeros((k, n), np.uint64), np.zeros((k, n), np.float32)
    pred, hop = np.zeros((k, n), np.uint32), np.zeros((k, n), np.uint32)
    _capi.check(net.ctx.handle, _capi.load().sg_routing_build_tree(
        net.ctx.handle, net._ensure_net(), nodes.ctypes.data, n, r0, r1, _capi.SG_ROUTE_SHORTEST_PATH,
        lat.ctypes.data, loss.ctypes.data, pred.ctypes.data, hop.ctypes.data))
    return pred


def _sentinels(net):
    return np.full(len(net.links()[0]), SENT, np.uint64), np.full(net.n_nodes, SENT, np.uint64)


def _raw(net, nodes, r0, r1, pred, counts, link, node, count_cols=None, n_nodes=None):
    """sg_link_load with host arrays; returns the status."""
    from shadow_amd import _capi

    nodes = np.ascontiguousarray(nodes, np.uint32)
    pred = np.ascontiguousarray(pred, np.uint32)
    counts = np.ascontiguousarray(counts, np.uint64)
    cols = counts.shape[1] if count_cols is None else count_cols
    return _capi.load().sg_link_load(
        net.ctx.handle, net._ensure_net(), nodes.ctypes.data, len(nodes) if n_nodes is None else n_nodes, r0, r1, 0,
        pred.ctypes.data, counts.ctypes.data, cols, None if link is None else link.ctypes.data,
        None if node is None else node.ctypes.data)


def _load(net, nodes, r0, r1, pred, counts, link, node):
    from shadow_amd import _capi

    _capi.check(net.ctx.handle, _raw(net, nodes, r0, r1, pred, counts, link, node))


def _lds_rows(ctx):
    """(rows the last call launched on the LDS path, the LDS path's node limit); timers on."""
    _, rows, n_max = ctx.read_timer("link_lds")
    return int(rows), int(n_max)


def _check(g, net, nodes, r0, r1, pred, counts):
    """One call from sentinels against the reference; returns the reference (link, node)."""
    link, node = _sentinels(net)
    _load(net, nodes, r0, r1, pred, counts, link, node)
    wl, wn = LR.link_load(g, nodes, (r0, r1), pred, counts)
    with np.errstate(over="ignore"):
        assert np.array_equal(link, wl + SENT), f"link loads differ on {int((link != wl + SENT).sum())} links"
        assert np.array_equal(node, wn + SENT), f"node loads differ on {int((node != wn + SENT).sum())} nodes"
    return wl, wn


@pytest.fixture(scope="module")
def tie(ctx):
    """(a)'s graph, its net and its pred rows, computed once."""
    g = LC.tie_graph()
    nodes = np.arange(g["n"], dtype=np.uint32)
    net = _net(g, ctx)
    return dict(g=g, nodes=nodes, net=net, pred=_pred(net, nodes, 0, g["n"]), dense=LC.dense_matrix(300, 300))


def test_dense_matrix_lds_path(ctx, tie):
    """(a)"""
    g, net = tie["g"], tie["net"]
    tail, head, _ = LR.links(g)
    gt, gh = net.links()
    assert np.array_equal(gt, tail) and np.array_equal(gh, head)
    fwd, rev = net.edge_links()
    wf, wr = LR.edge_links(g)
    assert np.array_equal(fwd, wf) and np.array_equal(rev, wr)
    ctx.enable_timers(True)
    try:
        wl, _ = _check(g, net, tie["nodes"], 0, 300, tie["pred"], tie["dense"])
        assert _lds_rows(ctx)[0] == 300
        assert ctx.read_timer("link_load")[1] == 1
    finally:
        ctx.enable_timers(False)
    assert int(wl[tail == head].sum()) == int(np.diag(tie["dense"]).sum())


def test_sparse_matrix_and_single_outputs(ctx, tie):
    """(b)"""
    g, net = tie["g"], tie["net"]
    c = LC.sparse_matrix()
    wl, wn = _check(g, net, tie["nodes"], 0, 300, tie["pred"], c)
    link, node = _sentinels(net)
    _load(net, tie["nodes"], 0, 300, tie["pred"], c, link, None)
    _load(net, tie["nodes"], 0, 300, tie["pred"], c, None, node)
    assert np.array_equal(link, wl + SENT) and np.array_equal(node, wn + SENT)


def test_used_subset_in_two_calls(ctx, tie):
    """(c)"""
    g, net = tie["g"], tie["net"]
    nodes = np.random.default_rng(21).permutation(300).astype(np.uint32)
    pred = _pred(net, nodes, 0, 120)
    c = LC.dense_matrix(120, 120, seed=22)
    wl, wn = _check(g, net, nodes, 0, 120, pred, c)
    link, node = _sentinels(net)
    _load(net, nodes, 0, 50, pred[:50], c[:50], link, node)
    _load(net, nodes, 50, 120, pred[50:], c[50:], link, node)
    assert np.array_equal(link, wl + SENT) and np.array_equal(node, wn + SENT)
    # nothing was attributed past the used columns' paths: the totals are the matrix's
    tail, head, _ = LR.links(g)
    assert int(wl[tail == head].sum()) == int(np.diag(c).sum())


def test_directed(ctx):
    """(d)"""
    g = LC.directed_graph()
    n = g["n"]
    net = _net(g, ctx)
    nodes = np.arange(n, dtype=np.uint32)
    fwd, rev = net.edge_links()
    assert (rev == UMAX).all() and np.array_equal(fwd, LR.edge_links(g)[0])
    tail, head = net.links()
    pairs = set(zip(tail.tolist(), head.tolist()))
    assert any((v, u) not in pairs for u, v in pairs)
    _check(g, net, nodes, 0, n, _pred(net, nodes, 0, n), LC.dense_matrix(n, n, seed=23))


def test_multigraph(ctx):
    """(e)"""
    g = LC.multi_graph()
    net = _net(g, ctx)
    nodes = np.arange(64, dtype=np.uint32)
    c = LC.dense_matrix(64, 64, seed=24)
    pred = _pred(net, nodes, 0, 64)
    wl, _ = _check(g, net, nodes, 0, 64, pred, c)
    tail, head = net.links()
    fwd, rev = net.edge_links()
    assert np.array_equal(tail[fwd], g["src"]) and np.array_equal(head[fwd], g["dst"])
    assert np.array_equal(tail[rev], g["dst"]) and np.array_equal(head[rev], g["src"])
    assert len(np.unique(fwd)) < len(fwd)  # parallel edges share a link
    # the diagonal alone: on the self-loop links and nowhere else
    link, _ = _sentinels(net)
    link[:] = 0
    _load(net, nodes, 0, 64, pred, np.diag(np.diag(c)), link, None)
    loops = tail == head
    assert np.array_equal(link[loops], np.diag(c)[head[loops]]) and not link[~loops].any()
    # per-edge loads: both directions of an edge's pair
    per_edge = np.where(fwd == rev, wl[fwd], wl[fwd] + wl[rev])
    k = int(np.flatnonzero(g["src"] != g["dst"])[0])
    assert per_edge[k] == wl[fwd[k]] + wl[rev[k]]
    same = (g["src"] == g["src"][k]) & (g["dst"] == g["dst"][k])
    assert (per_edge[same] == per_edge[k]).all()


@pytest.mark.parametrize("which", ["path", "star"])
def test_shape_extremes(ctx, which):
    """(f)"""
    if which == "path":
        g = LC.path_graph(4096)
        net = _net(g, ctx)
        nodes = np.arange(4096, dtype=np.uint32)
        tail, head, keys = LR.links(g)
        up = LR.link_index(keys, np.arange(4095), np.arange(1, 4096))    # the links (v - 1 -> v)
        down = LR.link_index(keys, np.arange(1, 4096), np.arange(4095))  # the links (v + 1 -> v)
        loop = LR.link_index(keys, np.arange(4096), np.arange(4096))
        for r0 in (0, 2016):  # the source at one end, and around the middle
            pred = _pred(net, nodes, r0, r0 + 64)
            # sparse traffic against the reference's walk
            _check(g, net, nodes, r0, r0 + 64, pred, LC.packet_matrix(64, 4096, 3000, seed=25))
            # dense traffic against the path's closed form: what crosses (v - 1 -> v) from source i < v
            # is the row's sum from column v on, and likewise downwards
            c = LC.dense_matrix(64, 4096, seed=25)
            link, node = _sentinels(net)
            _load(net, nodes, r0, r0 + 64, pred, c, link, node)
            wl, wn = np.zeros(len(keys), np.uint64), np.zeros(4096, np.uint64)
            for i in range(64):
                s = r0 + i
                suffix = np.cumsum(c[i, ::-1])[::-1]  # suffix[v] = the sum of columns v ..
                prefix = np.cumsum(c[i])              # prefix[v] = the sum of columns .. v
                wl[up[s:]] += suffix[s + 1:]
                wn[s + 1:] += suffix[s + 1:]
                wl[down[:s]] += prefix[:s]
                wn[:s] += prefix[:s]
                wl[loop[s]] += c[i, s]
            assert np.array_equal(link, wl + SENT) and np.array_equal(node, wn + SENT)
    else:
        g = LC.star_graph()
        net = _net(g, ctx)
        nodes = np.arange(513, dtype=np.uint32)
        pred = _pred(net, nodes, 0, 513)
        assert int((pred[1] == 0).sum()) >= 500  # the hub's children in a spoke's row
        _check(g, net, nodes, 0, 513, pred, LC.dense_matrix(513, 513, seed=26))


def test_forced_global_path(ctx, tie, monkeypatch):
    """(g): SG_LINK_LDS=0 gives the LDS path's result."""
    g, net = tie["g"], tie["net"]
    monkeypatch.setenv("SG_LINK_LDS", "0")
    ctx.enable_timers(True)
    try:
        _check(g, net, tie["nodes"], 0, 300, tie["pred"], tie["dense"])
        assert _lds_rows(ctx)[0] == 0
    finally:
        ctx.enable_timers(False)


def test_lds_limit(ctx):
    """(g): the largest n the LDS path takes (read from the timer), and n + 1."""
    ctx.enable_timers(True)
    try:
        g0 = LC.sparse_graph(64)
        n0 = np.arange(64, dtype=np.uint32)
        net0 = _net(g0, ctx)
        _check(g0, net0, n0, 0, 8, _pred(net0, n0, 0, 8), LC.dense_matrix(8, 64))
        n_max = _lds_rows(ctx)[1]
        assert 4096 <= n_max < 65535
        for n, lds_rows in ((n_max, 64), (n_max + 1, 0)):
            g = LC.sparse_graph(n)
            nodes = np.arange(n, dtype=np.uint32)
            net = _net(g, ctx)
            r0 = n // 2 - 32
            pred = _pred(net, nodes, r0, r0 + 64)
            link, node = _sentinels(net)
            c = LC.packet_matrix(64, n, 20000, seed=27)
            _load(net, nodes, r0, r0 + 64, pred, c, link, node)
            assert _lds_rows(ctx)[0] == lds_rows, n
            wl, wn = LR.link_load(g, nodes, (r0, r0 + 64), pred, c)
            assert np.array_equal(link, wl + SENT) and np.array_equal(node, wn + SENT)
    finally:
        ctx.enable_timers(False)


def test_c3_shape(ctx):
    """(h): rows [0, 512) of the C3 shape, 50,000 packets on random pairs of those rows."""
    g = LC.c3_graph()
    nodes = np.arange(10000, dtype=np.uint32)
    net = _net(g, ctx)
    pred = _pred(net, nodes, 0, 512)
    c = LC.packet_matrix(512, 10000, 50000)
    ctx.enable_timers(True)
    try:
        _check(g, net, nodes, 0, 512, pred, c)
        assert _lds_rows(ctx)[0] == 512
    finally:
        ctx.enable_timers(False)


def test_end_to_end_round(ctx, tie):
    """(i): a delivery round counts on the device; sg_link_load folds those counters device to
    device; the reference works from the round's own statuses and the hosts' route rows."""
    import torch

    from shadow_amd import _capi, synth
    from shadow_amd.worker import DeviceTable, HostTable, PacketBatch, deliver_round

    g, net, nodes, n = tie["g"], tie["net"], tie["nodes"], 300
    dlat = torch.zeros((n, n), dtype=torch.int64, device="cuda")
    dloss = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    dpred = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    net.build_rows_device(nodes, 0, n, dlat.data_ptr(), dloss.data_ptr())
    net.tree_rows_device(nodes, 0, n, dlat.data_ptr(), dloss.data_ptr(), dpred.data_ptr(), 0)
    hosts = synth.make_hosts(1000, n)
    t0 = 946684800 * 10**9
    pk = synth.make_packets(20000, hosts, t0, t0 + 10**6, seed=31)
    ht = HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=ctx)
    counts = torch.zeros(n * n, dtype=torch.int64, device="cuda")
    ctx.set_packet_counters(counts)
    try:
        out = deliver_round(ht, DeviceTable(dlat.ravel(), dloss.ravel(), n),
                            PacketBatch.from_numpy(pk["src"], pk["dst_ip"], pk["payload"], pk["send_time"]),
                            t0 + 10**6, 2**63, 0, ctx=ctx)
        status = out.to_numpy(len(pk["src"]))["status"]
    finally:
        ctx.set_packet_counters(None)
    n_links = len(net.links()[0])
    dlink = torch.full((n_links,), 5, dtype=torch.int64, device="cuda")
    dnode = torch.full((n,), 9, dtype=torch.int64, device="cuda")
    net.link_load_device(nodes, 0, n, dpred.data_ptr(), counts.data_ptr(), n, dlink.data_ptr(), dnode.data_ptr())
    torch.cuda.synchronize()
    dlv = np.flatnonzero(status == _capi.SG_PKT_DELIVERED)
    assert 0 < len(dlv) <= 20000
    ip_to_host = {int(ip): h for h, ip in enumerate(hosts["ip"])}
    dh = np.array([ip_to_host[int(x)] for x in pk["dst_ip"][dlv]], np.int64)
    want = np.zeros((n, n), np.uint64)
    np.add.at(want, (hosts["route"][pk["src"][dlv]].astype(np.int64), hosts["route"][dh].astype(np.int64)),
              np.uint64(1))
    assert np.array_equal(counts.cpu().numpy().view(np.uint64).reshape(n, n), want)
    wl, wn = LR.link_load(g, nodes, (0, n), tie["pred"], want)
    assert np.array_equal(dlink.cpu().numpy().view(np.uint64), wl + np.uint64(5))
    assert np.array_equal(dnode.cpu().numpy().view(np.uint64), wn + np.uint64(9))
    tail, head, _ = LR.links(g)
    assert int(wl[tail == head].sum()) + int(wn.sum()) >= len(dlv)


def test_corrupted_pred(ctx, tie):
    """(j): SG_ERR_INVALID_ARG with the first (row, col); the call returns."""
    from shadow_amd import _capi

    g, net, nodes = tie["g"], tie["net"], tie["nodes"]
    n = g["n"]
    pred, c = tie["pred"][:16], tie["dense"][:16]
    _, _, keys = LR.links(g)

    def run(p, counts=c):
        link, node = _sentinels(net)
        rc = _raw(net, nodes, 0, 16, p, counts, link, node)
        r, k = _capi.C.c_uint32(), _capi.C.c_uint32()
        _capi.load().sg_ctx_last_error_pair(ctx.handle, _capi.C.byref(r), _capi.C.byref(k))
        msg = _capi.load().sg_ctx_last_error(ctx.handle).decode()
        return rc, (r.value, k.value), msg

    cases = []
    p = pred.copy()  # a 2-cycle in row 7
    a = 40
    b = int(p[7, a])
    assert b != 7
    p[7, b] = a
    cases.append((p, "cycle"))
    p = pred.copy()  # a value >= n
    p[5, 123] = n
    cases.append((p, "range"))
    p = pred.copy()  # a pair that is not a link
    v = 200


    def above(x):  # the nodes from x up to row 3's source
        seen = [x]
        while seen[-1] != 3:
            seen.append(int(pred[3, seen[-1]]))
        return seen

    # (u outside v's subtree: the row stays a tree, only the pair is wrong)
    u = next(x for x in range(n) if x != v and LR.link_index(keys, [x], [v])[0] < 0 and v not in above(x))
    p[3, v] = u
    cases.append((p, "link"))
    p = pred.copy()  # pred[s] != s
    p[9, 9] = 10
    cases.append((p, "source"))
    for p, word in cases:
        want = LR.first_bad(g, nodes, (0, 16), p, c)
        assert want is not None
        rc, pair, msg = run(p)
        assert rc == _capi.SG_ERR_INVALID_ARG and pair == want and word in msg, (word, pair, want, msg)
    # the same corrupted row under an all-zero counter row is skipped, as documented
    c0 = c.copy()
    c0[9] = 0
    rc, _, _ = run(cases[3][0], c0)
    assert rc == _capi.SG_OK
    # and the context still works
    _check(g, net, nodes, 0, 16, pred, c)


def test_argument_errors(ctx, tie):
    """(k): SG_ERR_INVALID_ARG, the sentinel outputs untouched."""
    from shadow_amd import _capi

    g, net, nodes = tie["g"], tie["net"], tie["nodes"]
    n = g["n"]
    pred, c = tie["pred"][:4], tie["dense"][:4]
    link, node = _sentinels(net)
    dup = nodes.copy()
    dup[5] = 6
    out = nodes.copy()
    out[9] = n
    L, h, nh = _capi.load(), ctx.handle, net._ensure_net()
    P, Cn, Lk, Nd, Ns = pred.ctypes.data, c.ctypes.data, link.ctypes.data, node.ctypes.data, nodes.ctypes.data
    bad = [_raw(net, dup, 0, 4, pred, c, link, node), _raw(net, out, 0, 4, pred, c, link, node),
           _raw(net, nodes[:40], 0, 4, pred, c, link, node), _raw(net, nodes, 3, 2, pred, c, link, node),
           _raw(net, nodes, n - 1, n + 1, pred, c, link, node), _raw(net, nodes, 0, 4, pred, c, None, None),
           _raw(net, nodes, 0, 4, pred, c, link, node, count_cols=n + 1),
           L.sg_link_load(h, nh, None, n, 0, 4, 0, P, Cn, n, Lk, Nd), L.sg_link_load(h, nh, Ns, n, 0, 4, 0, None, Cn, n, Lk, Nd),
           L.sg_link_load(h, nh, Ns, n, 0, 4, 0, P, None, n, Lk, Nd), L.sg_link_load(h, None, Ns, n, 0, 4, 0, P, Cn, n, Lk, Nd)]
    assert bad == [_capi.SG_ERR_INVALID_ARG] * len(bad)
    assert (link == SENT).all() and (node == SENT).all()
    # sg_net_links: the count alone, a short buffer, then the list
    k = _capi.C.c_uint32()
    t, hd = np.full(4, UMAX, np.uint32), np.full(4, UMAX, np.uint32)
    assert L.sg_net_links(h, nh, _capi.C.byref(k), t.ctypes.data, hd.ctypes.data, 4) == _capi.SG_ERR_CAPACITY
    assert k.value == len(link) and (t == UMAX).all() and (hd == UMAX).all()
    # an empty row range is fine and adds nothing
    assert _raw(net, nodes, 2, 2, pred, c, link, node) == _capi.SG_OK
    assert (link == SENT).all() and (node == SENT).all()


def test_python_interface(ctx, tie):
    """(l): PathTree.link_load and NetworkGraph.links."""
    g, net = tie["g"], tie["net"]
    t = net.compute_shortest_path_tree([7, 3, 250])
    c = LC.dense_matrix(3, 120, seed=28)
    link, node = t.link_load(c)
    wl, wn = LR.link_load(g, t.nodes, (0, 3), t.pred, c)
    assert link.dtype == np.uint64 and np.array_equal(link, wl) and np.array_equal(node, wn)
    tail, head = net.links()
    assert len(link) == len(tail) and np.all((head[1:] > head[:-1]) | ((head[1:] == head[:-1]) & (tail[1:] > tail[:-1])))
    with pytest.raises(ValueError):
        t.link_load(np.zeros((2, 300), np.uint64))
