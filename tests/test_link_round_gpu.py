"""Link loads from a round's packets on the GPU (sg_link_load_packets, PathTree.link_load_round).

In every case the pred rows come from sg_routing_build_tree on the same net: their own
correctness is test_tree_gpu.py's, here they are inputs.  The outputs start from sentinels, so
that "adds into" (and "every hops entry is written") is itself checked, and every comparison with
tests/link_round_ref.py is exact (np.array_equal on u64 / u32).  The inputs' own conditions are
checked on the CPU in test_link_round_ref_cpu.py."""
import numpy as np
import pytest

import link_cases as LC
import link_ref as LR
import link_round_cases as RC
import link_round_ref as RR

pytestmark = pytest.mark.gpu

SENT, SENT32, UMAX = RC.SENT64, RC.SENT32, 0xFFFFFFFF


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


def _host_table(hosts, ctx):
    from shadow_amd.worker import HostTable

    return HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=ctx)


def _batch(pk):
    from shadow_amd.worker import PacketBatch

    n = len(pk["src"])
    return PacketBatch.from_numpy(pk["src"], pk["dst_ip"], pk.get("payload", np.zeros(n, np.uint32)),
                                  pk.get("send_time", np.zeros(n, np.uint64)))


def _dev(x, view):
    import torch

    return None if x is None else torch.from_numpy(np.ascontiguousarray(x).view(view)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _sentinels(net, n_packets):
    return (np.full(len(net.links()[0]), SENT, np.uint64), np.full(net.n_nodes, SENT, np.uint64),
            np.full(n_packets, SENT32, np.uint32))


def _raw(net, ht, nodes, r0, r1, pred, pb, status, weight, link, node, hops, n_nodes=None):
    """sg_link_load_packets with host pred and outputs (status / weight: device tensors or None);
    returns the status code."""
    from shadow_amd import _capi

    nodes = np.ascontiguousarray(nodes, np.uint32)
    pred = np.ascontiguousarray(pred, np.uint32)
    p = pb.c_struct()
    return _capi.load().sg_link_load_packets(
        net.ctx.handle, net._ensure_net(), ht.handle, nodes.ctypes.data, len(nodes) if n_nodes is None else n_nodes,
        r0, r1, 0, pred.ctypes.data, _capi.C.byref(p), _ptr(status), _ptr(weight),
        None if link is None else link.ctypes.data, None if node is None else node.ctypes.data,
        None if hops is None else hops.ctypes.data)


def _error(ctx):
    from shadow_amd import _capi

    r, k = _capi.C.c_uint32(), _capi.C.c_uint32()
    _capi.load().sg_ctx_last_error_pair(ctx.handle, _capi.C.byref(r), _capi.C.byref(k))
    return (r.value, k.value), _capi.load().sg_ctx_last_error(ctx.handle).decode()


def _check(g, net, ht, nodes, rows, pred, hosts, pk, status=None, weight=None, pb=None):
    """One call from sentinels against the reference; returns the reference (link, node, hops)."""
    from shadow_amd import _capi

    pb = pb or _batch(pk)
    link, node, hops = _sentinels(net, len(pk["src"]))
    _capi.check(net.ctx.handle, _raw(net, ht, nodes, rows[0], rows[1], pred, pb, _dev(status, np.uint8),
                                     _dev(weight, np.int32), link, node, hops))
    wl, wn, wh = RR.link_load_round(g, nodes, rows, pred, hosts, pk, status, weight)
    with np.errstate(over="ignore"):
        assert np.array_equal(link, wl + SENT), f"link loads differ on {int((link != wl + SENT).sum())} links"
        assert np.array_equal(node, wn + SENT), f"node loads differ on {int((node != wn + SENT).sum())} nodes"
    assert np.array_equal(hops, wh), f"hops differ on {int((hops != wh).sum())} packets"
    return wl, wn, wh


@pytest.fixture(scope="module")
def tie(ctx):
    """(a)'s graph, net, pred rows, hosts and batch, computed once."""
    g = LC.tie_graph()
    nodes = np.arange(g["n"], dtype=np.uint32)
    net = _net(g, ctx)
    hosts, pk = RC.tie_round()
    return dict(g=g, nodes=nodes, net=net, pred=_pred(net, nodes, 0, g["n"]), hosts=hosts, pk=pk,
                ht=_host_table(hosts, ctx), pb=_batch(pk))


@pytest.fixture(scope="module")
def tie_status(ctx, tie):
    """(a)'s delivery round with device counters on: (device status, device counters, device pred)."""
    import torch

    from shadow_amd.worker import DeviceTable, deliver_round

    net, nodes, n = tie["net"], tie["nodes"], 300
    dlat = torch.zeros((n, n), dtype=torch.int64, device="cuda")
    dloss = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    dpred = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    net.build_rows_device(nodes, 0, n, dlat.data_ptr(), dloss.data_ptr())
    net.tree_rows_device(nodes, 0, n, dlat.data_ptr(), dloss.data_ptr(), dpred.data_ptr(), 0)
    counts = torch.zeros(n * n, dtype=torch.int64, device="cuda")
    ctx.set_packet_counters(counts)
    try:
        # (a host table of its own: the round advances its hosts' streams)
        out = deliver_round(_host_table(tie["hosts"], ctx), DeviceTable(dlat.ravel(), dloss.ravel(), n), tie["pb"],
                            RC.ROUND_END, 2**63, 0, ctx=ctx)
    finally:
        ctx.set_packet_counters(None)
    return dict(out=out, counts=counts, dpred=dpred)


def test_round_three_ways(ctx, tie, tie_status):
    """(a): device to device on the round's own status = the reference = sg_link_load folded from
    the round's counters."""
    import torch

    g, net, nodes, n = tie["g"], tie["net"], tie["nodes"], 300
    out, counts, dpred = tie_status["out"], tie_status["counts"], tie_status["dpred"]
    npk = len(tie["pk"]["src"])
    status = out.status[:npk].cpu().numpy()
    assert np.array_equal(dpred.cpu().numpy().view(np.uint32), tie["pred"])
    n_links = len(net.links()[0])
    dlink = torch.full((n_links,), 5, dtype=torch.int64, device="cuda")
    dnode = torch.full((n,), 9, dtype=torch.int64, device="cuda")
    dhops = torch.full((npk,), 77, dtype=torch.int32, device="cuda")
    ctx.enable_timers(True)
    try:
        net.link_load_packets_device(tie["ht"], nodes, 0, n, dpred.data_ptr(), tie["pb"], out.status.data_ptr(), 0,
                                     dlink.data_ptr(), dnode.data_ptr(), dhops.data_ptr())
        assert ctx.read_timer("link_packets")[1] == 1
        assert int(ctx.read_timer("link_packets_counted")[1]) == int((status == 0).sum()) == out.n_delivered
        assert int(ctx.read_timer("link_packets")[2]) == out.n_delivered
    finally:
        ctx.enable_timers(False)
    wl, wn, wh = RR.link_load_round(g, nodes, (0, n), tie["pred"], tie["hosts"], tie["pk"], status)
    got_l, got_n = dlink.cpu().numpy().view(np.uint64), dnode.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_l, wl + np.uint64(5)) and np.array_equal(got_n, wn + np.uint64(9))
    assert np.array_equal(dhops.cpu().numpy().view(np.uint32), wh)
    # the dense fold of the round's own counters
    flink = torch.full((n_links,), 5, dtype=torch.int64, device="cuda")
    fnode = torch.full((n,), 9, dtype=torch.int64, device="cuda")
    net.link_load_device(nodes, 0, n, dpred.data_ptr(), counts.data_ptr(), n, flink.data_ptr(), fnode.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(got_l, flink.cpu().numpy().view(np.uint64))
    assert np.array_equal(got_n, fnode.cpu().numpy().view(np.uint64))
    assert int(wl.sum()) > out.n_delivered > 0


def test_weights_and_single_outputs(ctx, tie, tie_status):
    """(b): payloads up to 2^32 - 1; each output alone."""
    from shadow_amd import _capi

    g, net, nodes, pk = tie["g"], tie["net"], tie["nodes"], tie["pk"]
    npk = len(pk["src"])
    status = tie_status["out"].status[:npk].cpu().numpy()
    w = RC.big_weights(npk)
    wl, wn, wh = _check(g, net, tie["ht"], nodes, (0, 300), tie["pred"], tie["hosts"], pk, status, w, pb=tie["pb"])
    assert int(wl.max()) >= 1 << 32
    dst, dw = _dev(status, np.uint8), _dev(w, np.int32)
    for which in range(3):
        outs = list(_sentinels(net, npk))
        args = [o if k == which else None for k, o in enumerate(outs)]
        _capi.check(ctx.handle, _raw(net, tie["ht"], nodes, 0, 300, tie["pred"], tie["pb"], dst, dw, *args))
        with np.errstate(over="ignore"):
            assert np.array_equal(outs[which], (wl + SENT, wn + SENT, wh)[which]), which


def test_statuses(ctx, tie):
    """(c): synthetic statuses with all four values, and status = NULL."""
    g, net, nodes, pk = tie["g"], tie["net"], tie["nodes"], tie["pk"]
    st = RC.mixed_status(len(pk["src"]))
    _, _, wh = _check(g, net, tie["ht"], nodes, (0, 300), tie["pred"], tie["hosts"], pk, st, pk["payload"], pb=tie["pb"])
    assert np.array_equal(wh == UMAX, st != 0)
    _, _, wh = _check(g, net, tie["ht"], nodes, (0, 300), tie["pred"], tie["hosts"], pk, None, None, pb=tie["pb"])
    assert (wh != UMAX).all()


@pytest.mark.parametrize("combine", ["0", "1"])
def test_combine_forms(ctx, tie, monkeypatch, combine):
    """SG_LINK_COMBINE=1 (the default: a wave sums its equal pairs before the walk) and 0 (every
    packet walks on its own) give the same arrays: on (c)'s statuses with weights up to 2^32 - 1,
    and on a batch that repeats each host's first packet."""
    g, net, nodes, pk = tie["g"], tie["net"], tie["nodes"], tie["pk"]
    monkeypatch.setenv("SG_LINK_COMBINE", combine)
    _check(g, net, tie["ht"], nodes, (0, 300), tie["pred"], tie["hosts"], pk, RC.mixed_status(len(pk["src"])),
           RC.big_weights(len(pk["src"])), pb=tie["pb"])
    first = np.searchsorted(pk["src"], pk["src"])  # (grouped by source host: the host's first packet)
    rep = dict(pk, dst_ip=pk["dst_ip"][first])
    _, _, wh = _check(g, net, tie["ht"], nodes, (0, 300), tie["pred"], tie["hosts"], rep, None, pk["payload"])
    assert len(np.unique(rep["dst_ip"])) < 1000 and (wh != UMAX).all()


def test_shuffled_nodes_two_row_blocks(ctx, tie):
    """(d): each block's call with its own pred block and its half of the batch, into one array."""
    from shadow_amd import _capi

    g, net = tie["g"], tie["net"]
    nodes, hosts, lo, hi = RC.shuffled_round()
    ht = _host_table(hosts, ctx)
    link, node, _ = _sentinels(net, 0)
    wl, wn = np.zeros(len(link), np.uint64), np.zeros(300, np.uint64)
    for (r0, r1), pk in (((0, 60), lo), ((60, 120), hi)):
        pred = _pred(net, nodes, r0, r1)
        hops = np.full(len(pk["src"]), SENT32, np.uint32)
        _capi.check(ctx.handle, _raw(net, ht, nodes, r0, r1, pred, _batch(pk), None, _dev(pk["payload"], np.int32),
                                     link, node, hops))
        _, _, wh = RR.link_load_round(g, nodes, (r0, r1), pred, hosts, pk, None, pk["payload"], wl, wn)
        assert np.array_equal(hops, wh)
    assert np.array_equal(link, wl + SENT) and np.array_equal(node, wn + SENT)
    assert wl.any() and wn.any()


@pytest.mark.parametrize("which", ["directed", "multi"])
def test_directed_and_multigraph(ctx, which):
    """(e): same-node packets land on self-loop links only; a general batch beside them."""
    g = LC.directed_graph() if which == "directed" else LC.multi_graph()
    n = g["n"]
    net = _net(g, ctx)
    nodes = np.arange(n, dtype=np.uint32)
    pred = _pred(net, nodes, 0, n)
    hosts, pk = RC.same_node_round(n)
    ht = _host_table(hosts, ctx)
    wl, wn, wh = _check(g, net, ht, nodes, (0, n), pred, hosts, pk, None, pk["payload"])
    tail, head = net.links()
    loops = tail == head
    assert (wh == 1).all() and not wn.any() and not wl[~loops].any()
    # per node: the bytes of its two hosts, gathered per edge through sg_net_edge_links
    fwd, rev = net.edge_links()
    self_edges = np.flatnonzero(g["src"] == g["dst"])
    per_node = np.zeros(n, np.uint64)
    np.add.at(per_node, hosts["route"][pk["src"]].astype(np.int64), pk["payload"].astype(np.uint64))
    assert np.array_equal(wl[fwd[self_edges]], per_node[g["src"][self_edges]])
    if which == "multi":
        assert np.array_equal(fwd[self_edges], rev[self_edges])
    pk2 = RC.batch(3000, hosts, 47)
    _check(g, net, ht, nodes, (0, n), pred, hosts, pk2, None, None)


@pytest.mark.parametrize("which", ["path", "star"])
def test_shape_extremes(ctx, which):
    """(f): a 4,095-hop walk; 3,000 packets over one link."""
    if which == "path":
        g, (hosts, pk), rows = LC.path_graph(4096), RC.path_round(), (0, 64)
    else:
        g, (hosts, pk), rows = LC.star_graph(512), RC.star_round(), (0, 8)
    net = _net(g, ctx)
    nodes = np.arange(g["n"], dtype=np.uint32)
    wl, _, wh = _check(g, net, _host_table(hosts, ctx), nodes, rows, _pred(net, nodes, *rows), hosts, pk)
    if which == "path":
        assert int(wh.max()) == 4095
    else:
        assert int(wl.max()) == 3000


def test_past_the_dense_folds_lds_limit(ctx):
    """(g): 11,667 nodes, rows [0, 64): the same kernel, no size limit."""
    g = LC.sparse_graph(11667)
    net = _net(g, ctx)
    nodes = np.arange(11667, dtype=np.uint32)
    hosts, pk = RC.block_round(64, 200, 5000, 49)
    _check(g, net, _host_table(hosts, ctx), nodes, (0, 64), _pred(net, nodes, 0, 64), hosts, pk, None, pk["payload"])


def test_c3_shape(ctx):
    """(h): rows [0, 512) of the C3 shape, 50,000 packets to hosts anywhere."""
    g = LC.c3_graph()
    net = _net(g, ctx)
    nodes = np.arange(10000, dtype=np.uint32)
    hosts, pk = RC.c3_round()
    _, _, wh = _check(g, net, _host_table(hosts, ctx), nodes, (0, 512), _pred(net, nodes, 0, 512), hosts, pk)
    assert int(wh.max()) > 8


def test_sparse_addresses(ctx, tie):
    """(i): the sorted address table resolves; packets to unknown addresses do not count."""
    hosts, pk, status = RC.sparse_address_round()
    _check(tie["g"], tie["net"], _host_table(hosts, ctx), tie["nodes"], (0, 300), tie["pred"], hosts, pk, status,
           pk["payload"])


def test_corrupted_pred(ctx, tie):
    """(j): SG_ERR_INVALID_ARG with the smallest (row, col); the call returns."""
    from shadow_amd import _capi

    g, net, nodes, hosts = tie["g"], tie["net"], tie["nodes"], tie["hosts"]
    n = g["n"]
    pred = tie["pred"]
    pk = {k: v[:3000] for k, v in tie["pk"].items()}
    pb = _batch(pk)
    _, _, keys = LR.links(g)
    _, ri, cj = RR.counted_pairs(hosts, pk, None)
    # a crossed cell: the destination of the first packet with two hops or more
    k = int(np.flatnonzero((ri != cj) & (pred[ri, cj] != ri))[0])
    i, j = int(ri[k]), int(cj[k])

    def run(p):
        link, node, hops = _sentinels(net, 3000)
        rc = _raw(net, tie["ht"], nodes, 0, n, p, pb, None, None, link, node, hops)
        return (rc,) + _error(ctx)

    def above(row, x):  # the nodes from x up to the row's source
        seen = [x]
        while seen[-1] != row:
            seen.append(int(pred[row, seen[-1]]))
        return seen

    cases = []
    p = pred.copy()  # a 2-cycle on that packet's path
    a = int(p[i, j])
    p[i, a] = j
    cases.append((p, "cycle"))
    p = pred.copy()  # a value >= n
    p[i, j] = n
    cases.append((p, "range"))
    p = pred.copy()  # a pair that is not a link
    u = next(x for x in range(n) if x != j and LR.link_index(keys, [x], [j])[0] < 0 and j not in above(i, x))
    p[i, j] = u
    cases.append((p, "link"))
    for p, word in cases:
        want = RR.first_bad_pred(g, nodes, (0, n), p, hosts, pk)
        assert want is not None and want[0] == i
        rc, pair, msg = run(p)
        assert rc == _capi.SG_ERR_INVALID_ARG and pair == want and word in msg, (word, pair, want, msg)
    # the same corruption in a cell no counted packet crosses succeeds
    crossed = np.zeros(n, bool)
    for c in cj[ri == i].tolist():
        if c != i:
            crossed[above(i, c)] = True
    free = int(np.flatnonzero(~crossed)[0])
    assert free != i
    for bad in (n, next(x for x in range(n) if x != free and LR.link_index(keys, [x], [free])[0] < 0)):
        p = pred.copy()
        p[i, free] = bad
        assert RR.first_bad_pred(g, nodes, (0, n), p, hosts, pk) is None
        assert run(p)[0] == _capi.SG_OK
    # and the context still works
    _check(g, net, tie["ht"], nodes, (0, n), pred, hosts, pk, pb=pb)


def test_packet_and_argument_errors(ctx, tie):
    """(k): device-side packet errors with their packet index; host-side argument errors leave
    the sentinels."""
    from shadow_amd import _capi

    g, net, nodes, hosts, ht = tie["g"], tie["net"], tie["nodes"], tie["hosts"], tie["ht"]
    n = g["n"]
    pred = tie["pred"]
    base = {k: v[:2000].copy() for k, v in tie["pk"].items()}
    st = np.zeros(2000, np.uint8)
    st[700] = RC.DROP_NO_DST

    def run(pk, status, r0=0, r1=n):
        link, node, hops = _sentinels(net, 2000)
        rc = _raw(net, ht, nodes, r0, r1, pred[r0:r1], _batch(pk), _dev(status, np.uint8), None, link, node, hops)
        return (rc,) + _error(ctx)

    # a source host out of range
    pk = dict(base, src=base["src"].copy())
    pk["src"][1234] = hosts["n"]
    rc, pair, msg = run(pk, st)
    assert rc == _capi.SG_ERR_INVALID_ARG and pair == (1234, UMAX) and "source host" in msg, (pair, msg)
    assert RR.first_bad_packet(hosts, pk, st, (0, n), n) == 1234
    # a source row outside the block
    want = RR.first_bad_packet(hosts, base, st, (0, 40), n)
    assert want is not None and want > 0
    rc, pair, msg = run(base, st, 0, 40)
    assert rc == _capi.SG_ERR_INVALID_ARG and pair == (want, UMAX) and "row" in msg, (pair, want, msg)
    # a counted packet to an unknown address; the uncounted one before it is passed over
    pk = dict(base, dst_ip=base["dst_ip"].copy())
    pk["dst_ip"][700] = pk["dst_ip"][900] = 0x0A090909
    rc, pair, msg = run(pk, st)
    assert rc == _capi.SG_ERR_INVALID_ARG and pair == (900, UMAX) and "address" in msg, (pair, msg)
    assert RR.first_bad_packet(hosts, pk, st, (0, n), n) == 900
    assert run(pk, None)[1] == (700, UMAX)
    # host-side argument errors
    link, node, hops = _sentinels(net, 2000)
    pb = _batch(base)
    dup = nodes.copy()
    dup[5] = 6
    other = _net(LC.multi_graph(), ctx)
    L, h, nh, p = _capi.load(), ctx.handle, net._ensure_net(), pb.c_struct()
    P, Lk, Nd, Hp, Ns, B = pred.ctypes.data, link.ctypes.data, node.ctypes.data, hops.ctypes.data, nodes.ctypes.data, \
        _capi.C.byref(p)
    bad = [_raw(net, ht, dup, 0, n, pred, pb, None, None, link, node, hops),
           _raw(net, ht, nodes[:40], 0, 4, pred, pb, None, None, link, node, hops),
           _raw(net, ht, nodes, 3, 2, pred, pb, None, None, link, node, hops),
           _raw(net, ht, nodes, n - 1, n + 1, pred, pb, None, None, link, node, hops),
           _raw(net, ht, nodes, 0, n, pred, pb, None, None, None, None, None),
           _raw(other, ht, nodes, 0, n, pred, pb, None, None, link, node, hops),
           L.sg_link_load_packets(h, None, ht.handle, Ns, n, 0, n, 0, P, B, None, None, Lk, Nd, Hp),
           L.sg_link_load_packets(h, nh, None, Ns, n, 0, n, 0, P, B, None, None, Lk, Nd, Hp),
           L.sg_link_load_packets(h, nh, ht.handle, None, n, 0, n, 0, P, B, None, None, Lk, Nd, Hp),
           L.sg_link_load_packets(h, nh, ht.handle, Ns, n, 0, n, 0, None, B, None, None, Lk, Nd, Hp),
           L.sg_link_load_packets(h, nh, ht.handle, Ns, n, 0, n, 0, P, None, None, None, Lk, Nd, Hp)]
    assert bad == [_capi.SG_ERR_INVALID_ARG] * len(bad)
    assert (link == SENT).all() and (node == SENT).all() and (hops == SENT32).all()
    # hops alone is an output
    assert _raw(net, ht, nodes, 0, n, pred, pb, None, None, None, None, hops) == _capi.SG_OK
    assert (hops != SENT32).all()


def test_python_interface(ctx, tie, tie_status):
    """(l): PathTree.link_load_round with weight="payload", from a Deliveries."""
    g, net, hosts, pk = tie["g"], tie["net"], tie["hosts"], tie["pk"]
    t = net.compute_shortest_path_tree()
    out = tie_status["out"]
    status = out.status[:len(pk["src"])].cpu().numpy()
    link, node, hops = t.link_load_round(tie["ht"], tie["pb"], out, "payload")
    wl, wn, wh = RR.link_load_round(g, t.nodes, (0, 300), t.pred, hosts, pk, status, pk["payload"])
    assert link.dtype == np.uint64 and hops.dtype == np.uint32
    assert np.array_equal(link, wl) and np.array_equal(node, wn) and np.array_equal(hops, wh)
    link, node, hops = t.link_load_round(tie["ht"], tie["pb"], status, pk["payload"])
    assert np.array_equal(link, wl) and np.array_equal(node, wn) and np.array_equal(hops, wh)
    link, _, hops = t.link_load_round(tie["ht"], tie["pb"])
    assert np.array_equal(link, RR.link_load_round(g, t.nodes, (0, 300), t.pred, hosts, pk)[0])
    with pytest.raises(ValueError):
        t.link_load_round(tie["ht"], tie["pb"], weight="bytes")
