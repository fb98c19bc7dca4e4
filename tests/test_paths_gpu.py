"""Batched tree paths on the GPU (sg_tree_paths, sg_tree_paths_packets, PathTree.paths,
PathTree.trace_round).

In every case the table and pred rows the library reads come from sg_routing_build_tree on the
same net: their own correctness is test_tree_gpu.py's, here they are inputs.  The reference
(tests/paths_ref.py) expands every path on the host and gathers latencies and losses from the
oracle's table.  Every output starts from sentinels, a few records longer than the total, so that
"nothing past the total is written" is itself checked; every comparison is exact (np.array_equal,
the f32 losses by their bits).  The inputs' own conditions are checked on the CPU in
test_paths_ref_cpu.py."""
import numpy as np
import pytest

import link_cases as LC
import link_ref as LR
import link_round_cases as RC
import link_round_ref as RR
import paths_cases as PC
import paths_ref as PR

pytestmark = pytest.mark.gpu

UMAX = 0xFFFFFFFF
PAD = 3  # sentinel records past the total
NAMES = ("node", "link", "lat", "loss")


def _net(g, ctx):
    from shadow_amd import NetworkGraph

    return NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)


def _tabs(net, nodes, r0, r1):
    """(pred, latency, loss) rows [r0, r1) from sg_routing_build_tree (host outputs)."""
    from shadow_amd import _capi

    nodes = np.ascontiguousarray(nodes, np.uint32)
    n, k = len(nodes), r1 - r0
    lat, loss = np.zeros((k, n), np.uint64), np.zeros((k, n), np.float32)
    pred, hop = np.zeros((k, n), np.uint32), np.zeros((k, n), np.uint32)
    _capi.check(net.ctx.handle, _capi.load().sg_routing_build_tree(
        net.ctx.handle, net._ensure_net(), nodes.ctypes.data, n, r0, r1, _capi.SG_ROUTE_SHORTEST_PATH,
        lat.ctypes.data, loss.ctypes.data, pred.ctypes.data, hop.ctypes.data))
    return pred, lat, loss


def _oracle_rows(O, g, nodes, r0, r1):
    rc, lat, loss, _ = O.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"],
                                        np.asarray(nodes, np.uint32), rows=(r0, r1), threads=8)
    assert rc == 0
    return lat, loss


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


def _sentinels(n_items, cap, which=NAMES):
    outs = dict(off=np.full(n_items + 1, PC.SENT_OFF, np.uint64), node=np.full(cap, PC.SENT32, np.uint32),
                link=np.full(cap, PC.SENT32, np.uint32), lat=np.full(cap, PC.SENT_LAT, np.uint64),
                loss=np.full(cap, PC.SENT_LOSS, np.float32))
    for k in NAMES:
        if k not in which:
            outs[k] = None
    return outs


def _untouched(outs):
    want = _sentinels(len(outs["off"]) - 1, max(len(v) for k, v in outs.items() if k != "off" and v is not None))
    return all(v is None or np.array_equal(v.view(np.uint8), want[k].view(np.uint8)) for k, v in outs.items())


def _call(net, nodes, r0, r1, tabs, outs, cap, pairs=None, ht=None, pb=None, status=None, dev=False, n_nodes=None):
    """One call of either entry point on numpy arrays: host-array mode, or (dev) everything
    uploaded, SG_ROUTE_OUT_DEVICE, and the outputs copied back into `outs`.  tabs = (pred,
    latency or None, loss or None); status: a device tensor or None.  Returns (status code, total)."""
    import torch

    from shadow_amd import _capi

    C = _capi.C
    nodes = np.ascontiguousarray(nodes, np.uint32)
    ins = [None if t is None else np.ascontiguousarray(t) for t in tabs]
    if pairs is not None:
        ins += [np.ascontiguousarray(pairs[0], np.uint32), np.ascontiguousarray(pairs[1], np.uint32)]
    keys = ("off",) + NAMES
    if dev:
        views = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.float32): np.float32}
        d_ins = [None if t is None else torch.from_numpy(t.view(views[t.dtype])).cuda() for t in ins]
        d_outs = {k: None if outs[k] is None else torch.from_numpy(outs[k].view(views[outs[k].dtype])).cuda()
                  for k in keys}
        ip = [None if t is None else C.c_void_p(t.data_ptr()) for t in d_ins]
        op = [None if d_outs[k] is None else C.c_void_p(d_outs[k].data_ptr()) for k in keys]
    else:
        ip = [None if t is None else t.ctypes.data for t in ins]
        op = [None if outs[k] is None else outs[k].ctypes.data for k in keys]
    total = C.c_uint64(0xDEAD)
    L, h = _capi.load(), net.ctx.handle
    nn = len(nodes) if n_nodes is None else n_nodes
    flags = _capi.SG_ROUTE_OUT_DEVICE if dev else 0
    if pairs is not None:
        rc = L.sg_tree_paths(h, net._ensure_net(), nodes.ctypes.data, nn, r0, r1, flags, ip[0], ip[1], ip[2],
                             len(ins[3]), ip[3], ip[4], *op, cap, C.byref(total))
    else:
        p = pb.c_struct()
        rc = L.sg_tree_paths_packets(h, net._ensure_net(), ht.handle, nodes.ctypes.data, nn, r0, r1, flags, ip[0],
                                     ip[1], ip[2], C.byref(p), None if status is None else C.c_void_p(status.data_ptr()),
                                     *op, cap, C.byref(total))
    if dev:
        torch.cuda.synchronize()
        for k in keys:
            if outs[k] is not None:
                outs[k][...] = d_outs[k].cpu().numpy().view(outs[k].dtype)
    return rc, total.value


def _error(ctx):
    from shadow_amd import _capi

    r, k = _capi.C.c_uint32(), _capi.C.c_uint32()
    _capi.load().sg_ctx_last_error_pair(ctx.handle, _capi.C.byref(r), _capi.C.byref(k))
    return (r.value, k.value), _capi.load().sg_ctx_last_error(ctx.handle).decode()


def _same(outs, want, which=NAMES):
    """The outputs against the reference (off, node, link, lat, loss); the tail still sentinels."""
    off, total = want[0], int(want[0][-1])
    assert np.array_equal(outs["off"], off), f"offsets differ at {int((outs['off'] != off).sum())} entries"
    tail = _sentinels(0, PAD)
    for k, w in zip(NAMES, want[1:]):
        if k not in which:
            continue
        got = outs[k]
        assert np.array_equal(got[:total].view(np.uint8), w.view(np.uint8)), \
            f"{k} differs at {int((got[:total] != w).sum())} of {total} records"
        assert np.array_equal(got[total:].view(np.uint8), tail[k][:len(got) - total].view(np.uint8)), f"{k}: written past the total"


def _check(net, nodes, rows, tabs, want, which=NAMES, **kw):
    """One call from sentinels at cap = the total against the reference."""
    from shadow_amd import _capi

    total = int(want[0][-1])
    outs = _sentinels(len(want[0]) - 1, total + PAD, which)
    rc, got_total = _call(net, nodes, rows[0], rows[1], tabs, outs, total, **kw)
    _capi.check(net.ctx.handle, rc)
    assert got_total == total
    _same(outs, want, which)
    return outs


@pytest.fixture(scope="module")
def tie(ctx, oracle):
    """The tie graph's net, its rows from the library and from the oracle, (a)'s hosts and batch."""
    g = LC.tie_graph()
    nodes = np.arange(g["n"], dtype=np.uint32)
    net = _net(g, ctx)
    hosts, pk = RC.tie_round()
    tabs = _tabs(net, nodes, 0, g["n"])
    olat, oloss = _oracle_rows(oracle, g, nodes, 0, g["n"])
    assert np.array_equal(tabs[1], olat) and np.array_equal(tabs[2].view(np.uint32), oloss.view(np.uint32))
    return dict(g=g, nodes=nodes, net=net, tabs=tabs, olat=olat, oloss=oloss, hosts=hosts, pk=pk,
                ht=_host_table(hosts, ctx), pb=_batch(pk))


def _want_packets(t, hosts, pk, status):
    return PR.packet_records(t["g"], t["nodes"], (0, 300), t["tabs"][0], t["olat"], t["oloss"], hosts, pk, status)


def test_round_device_to_device(ctx, tie):
    """(a): a delivery round's own status, everything on the device: the reference's arrays, the
    record counts of sg_link_load_packets' out_hops, and its byte loads from out_link."""
    import torch

    from shadow_amd.worker import DeviceTable, deliver_round

    g, net, nodes, pk, n = tie["g"], tie["net"], tie["nodes"], tie["pk"], 300
    npk = len(pk["src"])
    dlat = torch.zeros((n, n), dtype=torch.int64, device="cuda")
    dloss = torch.zeros((n, n), dtype=torch.float32, device="cuda")
    dpred = torch.zeros((n, n), dtype=torch.int32, device="cuda")
    net.build_rows_device(nodes, 0, n, dlat.data_ptr(), dloss.data_ptr())
    net.tree_rows_device(nodes, 0, n, dlat.data_ptr(), dloss.data_ptr(), dpred.data_ptr(), 0)
    # (a host table of its own: the round advances its hosts' streams)
    out = deliver_round(_host_table(tie["hosts"], ctx), DeviceTable(dlat.ravel(), dloss.ravel(), n), tie["pb"],
                        RC.ROUND_END, 2**63, 0, ctx=ctx)
    status = out.status[:npk].cpu().numpy()
    want = _want_packets(tie, tie["hosts"], pk, status)
    total = int(want[0][-1])
    assert 0 < total and int((status == 0).sum()) == out.n_delivered
    doff = torch.full((npk + 1,), -1, dtype=torch.int64, device="cuda")
    dnode = torch.full((total + PAD,), 77, dtype=torch.int32, device="cuda")
    dlink = torch.full((total + PAD,), 77, dtype=torch.int32, device="cuda")
    dl = torch.full((total + PAD,), 77, dtype=torch.int64, device="cuda")
    df = torch.full((total + PAD,), -7.5, dtype=torch.float32, device="cuda")
    ctx.enable_timers(True)
    try:
        got_total = net.tree_paths_packets_device(tie["ht"], nodes, 0, n, dpred.data_ptr(), dlat.data_ptr(),
                                                  dloss.data_ptr(), tie["pb"], out.status.data_ptr(), doff.data_ptr(),
                                                  dnode.data_ptr(), dlink.data_ptr(), dl.data_ptr(), df.data_ptr(), total)
        for name in ("tree_paths_count", "tree_paths_fill"):
            _, launches, work = ctx.read_timer(name)
            assert launches == 1 and int(work) == total, (name, launches, work)
    finally:
        ctx.enable_timers(False)
    torch.cuda.synchronize()
    assert got_total == total
    off = doff.cpu().numpy().view(np.uint64)
    assert np.array_equal(off, want[0])
    got = (dnode.cpu().numpy().view(np.uint32), dlink.cpu().numpy().view(np.uint32), dl.cpu().numpy().view(np.uint64),
           df.cpu().numpy())
    for k, a, w in zip(NAMES, got, want[1:]):
        assert np.array_equal(a[:total].view(np.uint8), w.view(np.uint8)), k
        assert (a[total:] == (-7.5 if k == "loss" else 77)).all(), k
    # sg_link_load_packets on the same inputs: hops and byte loads
    n_links = len(net.links()[0])
    dload = torch.zeros((n_links,), dtype=torch.int64, device="cuda")
    dhops = torch.zeros((npk,), dtype=torch.int32, device="cuda")
    net.link_load_packets_device(tie["ht"], nodes, 0, n, dpred.data_ptr(), tie["pb"], out.status.data_ptr(),
                                 tie["pb"].payload_len.data_ptr(), dload.data_ptr(), 0, dhops.data_ptr())
    torch.cuda.synchronize()
    hops = dhops.cpu().numpy().view(np.uint32)
    cnt = np.diff(off.astype(np.int64))
    assert np.array_equal(cnt, np.where(hops == UMAX, 0, hops))
    load = np.zeros(n_links, np.uint64)
    np.add.at(load, got[1][:total], np.repeat(pk["payload"].astype(np.uint64), cnt))
    assert np.array_equal(load, dload.cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("n_pairs", PC.PAIR_COUNTS)
def test_pair_form_both_fills(ctx, tie, monkeypatch, n_pairs):
    """(b): the pair form, device arrays; the direct fill, and the staged fill with the first
    wave's span one record under the capacity, at it, and one over (that wave then stores
    directly; at 257 pairs other waves lie on either side of each capacity)."""
    ri, cj = PC.tie_pairs(n_pairs)
    want = PR.records(tie["g"], tie["nodes"], (0, 300), tie["tabs"][0], tie["olat"], tie["oloss"], ri.astype(np.int64), cj)
    monkeypatch.setenv("SG_PATHS_STAGE", "0")
    _check(tie["net"], tie["nodes"], (0, 300), tie["tabs"], want, pairs=(ri, cj), dev=True)
    monkeypatch.setenv("SG_PATHS_STAGE", "1")
    monkeypatch.delenv("SG_PATHS_STAGE_HOPS", raising=False)
    _check(tie["net"], tie["nodes"], (0, 300), tie["tabs"], want, pairs=(ri, cj), dev=True)
    for hops in PC.stage_capacities(want[0]):
        monkeypatch.setenv("SG_PATHS_STAGE_HOPS", str(hops))
        _check(tie["net"], tie["nodes"], (0, 300), tie["tabs"], want, pairs=(ri, cj), dev=True)


@pytest.mark.parametrize("stage", ["0", "1"])
def test_each_output_alone(ctx, tie, monkeypatch, stage):
    """(c): each record output alone, the others NULL; latency without the loss rows and loss
    without the latency rows."""
    monkeypatch.setenv("SG_PATHS_STAGE", stage)
    pk = {k: v[:3000] for k, v in tie["pk"].items()}
    want = _want_packets(tie, tie["hosts"], pk, None)
    pred, lat, loss = tie["tabs"]
    for which, tabs in ((("node",), (pred, None, None)), (("link",), (pred, None, None)), (("lat",), (pred, lat, None)),
                        (("loss",), (pred, None, loss)), (("node", "loss"), (pred, lat, loss))):
        _check(tie["net"], tie["nodes"], (0, 300), tabs, want, which, ht=tie["ht"], pb=_batch(pk))


def test_statuses(ctx, tie):
    """(d): uncounted packets (no record) between counted ones; status = NULL."""
    pk = tie["pk"]
    st = RC.mixed_status(len(pk["src"]))
    want = _want_packets(tie, tie["hosts"], pk, st)
    assert np.array_equal(np.diff(want[0].astype(np.int64)) == 0, st != 0)
    _check(tie["net"], tie["nodes"], (0, 300), tie["tabs"], want, ht=tie["ht"], pb=tie["pb"], status=_dev(st, np.uint8))
    want = _want_packets(tie, tie["hosts"], pk, None)
    assert (np.diff(want[0].astype(np.int64)) > 0).all()
    _check(tie["net"], tie["nodes"], (0, 300), tie["tabs"], want, ht=tie["ht"], pb=tie["pb"])


def test_shuffled_nodes_two_row_blocks(ctx, tie, oracle):
    """(e): a shuffled node order; each row block's call with its own pred and table blocks."""
    g, net = tie["g"], tie["net"]
    nodes, hosts, lo, hi = RC.shuffled_round()
    ht = _host_table(hosts, ctx)
    for (r0, r1), pk in (((0, 60), lo), ((60, 120), hi)):
        tabs = _tabs(net, nodes, r0, r1)
        olat, oloss = _oracle_rows(oracle, g, nodes, r0, r1)
        want = PR.packet_records(g, nodes, (r0, r1), tabs[0], olat, oloss, hosts, pk)
        _check(net, nodes, (r0, r1), tabs, want, ht=ht, pb=_batch(pk))
        _check(net, nodes, (r0, r1), tabs, want, ht=ht, pb=_batch(pk), dev=True)


@pytest.mark.parametrize("which", ["directed", "multi"])
def test_directed_and_multigraph(ctx, oracle, which):
    """(e): same-node pairs give the self-loop record carrying the diagonal cell; a general batch
    beside them."""
    g = LC.directed_graph() if which == "directed" else LC.multi_graph()
    n = g["n"]
    net = _net(g, ctx)
    nodes = np.arange(n, dtype=np.uint32)
    tabs = _tabs(net, nodes, 0, n)
    olat, oloss = _oracle_rows(oracle, g, nodes, 0, n)
    hosts, pk = RC.same_node_round(n)
    ht = _host_table(hosts, ctx)
    want = PR.packet_records(g, nodes, (0, n), tabs[0], olat, oloss, hosts, pk)
    outs = _check(net, nodes, (0, n), tabs, want, ht=ht, pb=_batch(pk))
    tail, head = net.links()
    row = hosts["route"][pk["src"]].astype(np.int64)
    assert np.array_equal(outs["off"], np.arange(2 * n + 1, dtype=np.uint64))
    assert np.array_equal(outs["node"][:2 * n], row) and np.array_equal(tail[outs["link"][:2 * n]], row)
    assert np.array_equal(head[outs["link"][:2 * n]], row)
    assert np.array_equal(outs["lat"][:2 * n], olat[row, row])
    assert np.array_equal(outs["loss"][:2 * n].view(np.uint32), oloss[row, row].view(np.uint32))
    pk2 = RC.batch(3000, hosts, 47)
    want = PR.packet_records(g, nodes, (0, n), tabs[0], olat, oloss, hosts, pk2)
    _check(net, nodes, (0, n), tabs, want, ht=ht, pb=_batch(pk2))


@pytest.mark.parametrize("which", ["path", "star"])
def test_shape_extremes(ctx, oracle, which):
    """(f): a 4,095-record path, every wave's span past the staging capacity (the staged form
    stores directly); 3,000 paths over one link."""
    if which == "path":
        g, (hosts, pk), rows = LC.path_graph(4096), RC.path_round(), (0, 64)
    else:
        g, (hosts, pk), rows = LC.star_graph(512), RC.star_round(), (0, 8)
    net = _net(g, ctx)
    nodes = np.arange(g["n"], dtype=np.uint32)
    tabs = _tabs(net, nodes, *rows)
    olat, oloss = _oracle_rows(oracle, g, nodes, *rows)
    want = PR.packet_records(g, nodes, rows, tabs[0], olat, oloss, hosts, pk)
    cnt = np.diff(want[0].astype(np.int64))
    assert int(cnt.max()) == (4095 if which == "path" else 2)
    _check(net, nodes, rows, tabs, want, ht=_host_table(hosts, ctx), pb=_batch(pk))


def test_past_the_dense_folds_lds_limit(ctx, oracle):
    """(g): 11,667 nodes, rows [0, 64)."""
    g = LC.sparse_graph(11667)
    net = _net(g, ctx)
    nodes = np.arange(11667, dtype=np.uint32)
    hosts, pk = RC.block_round(64, 200, 5000, 49)
    tabs = _tabs(net, nodes, 0, 64)
    olat, oloss = _oracle_rows(oracle, g, nodes, 0, 64)
    want = PR.packet_records(g, nodes, (0, 64), tabs[0], olat, oloss, hosts, pk)
    _check(net, nodes, (0, 64), tabs, want, ht=_host_table(hosts, ctx), pb=_batch(pk))


def test_c3_shape(ctx, oracle):
    """(h): rows [0, 512) of the C3 shape, 50,000 packets to hosts anywhere."""
    g = LC.c3_graph()
    net = _net(g, ctx)
    nodes = np.arange(10000, dtype=np.uint32)
    hosts, pk = RC.c3_round()
    tabs = _tabs(net, nodes, 0, 512)
    olat, oloss = _oracle_rows(oracle, g, nodes, 0, 512)
    want = PR.packet_records(g, nodes, (0, 512), tabs[0], olat, oloss, hosts, pk)
    assert int(np.diff(want[0].astype(np.int64)).max()) > 8
    _check(net, nodes, (0, 512), tabs, want, ht=_host_table(hosts, ctx), pb=_batch(pk), dev=True)


def test_sparse_addresses(ctx, tie):
    """(i): the sorted address table resolves; packets to unknown addresses have no record."""
    hosts, pk, status = RC.sparse_address_round()
    want = _want_packets(tie, hosts, pk, status)
    _check(tie["net"], tie["nodes"], (0, 300), tie["tabs"], want, ht=_host_table(hosts, ctx), pb=_batch(pk),
           status=_dev(status, np.uint8))


@pytest.mark.parametrize("dev", [False, True])
def test_capacity(ctx, tie, dev):
    """(j): cap one below the total: SG_ERR_CAPACITY, out_off and *total complete, no record
    written; the second call at cap = total succeeds."""
    from shadow_amd import _capi

    ri, cj = PC.tie_pairs(257)
    want = PR.records(tie["g"], tie["nodes"], (0, 300), tie["tabs"][0], tie["olat"], tie["oloss"], ri.astype(np.int64), cj)
    total = int(want[0][-1])
    outs = _sentinels(257, total + PAD)
    rc, got = _call(tie["net"], tie["nodes"], 0, 300, tie["tabs"], outs, total - 1, pairs=(ri, cj), dev=dev)
    assert rc == _capi.SG_ERR_CAPACITY and got == total
    assert np.array_equal(outs["off"], want[0])
    assert _untouched(dict(outs, off=np.full(258, PC.SENT_OFF, np.uint64)))
    rc, got = _call(tie["net"], tie["nodes"], 0, 300, tie["tabs"], outs, total, pairs=(ri, cj), dev=dev)
    assert rc == _capi.SG_OK and got == total
    _same(outs, want)


def test_corrupted_pred(ctx, tie):
    """(k): a 2-cycle, a value >= n and a non-link on a walked path, each with its (row, col); a
    value >= n comes ahead of a non-link with a smaller (row, col); the same corruption in an
    unwalked cell succeeds."""
    from shadow_amd import _capi

    g, net, nodes, hosts = tie["g"], tie["net"], tie["nodes"], tie["hosts"]
    n = g["n"]
    pred, lat, loss = tie["tabs"]
    pk = {k: v[:3000] for k, v in tie["pk"].items()}
    pb = _batch(pk)
    _, _, keys = LR.links(g)
    _, ri, cj = RR.counted_pairs(hosts, pk, None)
    # a walked cell: the destination of the first packet with two hops or more
    k = int(np.flatnonzero((ri != cj) & (pred[ri, cj] != ri))[0])
    i, j = int(ri[k]), int(cj[k])

    def run(p, which=NAMES):
        outs = _sentinels(3000, 40000, which)
        rc, _ = _call(net, nodes, 0, n, (p, lat, loss), outs, 40000, ht=tie["ht"], pb=pb)
        return (rc,) + _error(ctx)

    def above(row, x):  # the nodes from x up to the row's source
        seen = [x]
        while seen[-1] != row:
            seen.append(int(pred[row, seen[-1]]))
        return seen

    def non_link(to, avoid):
        return next(x for x in range(n) if x != to and LR.link_index(keys, [x], [to])[0] < 0 and to not in above(i, x)
                    and x not in avoid)

    cases = []
    p = pred.copy()  # a 2-cycle on that packet's path
    p[i, int(p[i, j])] = j
    cases.append((p, "cycle"))
    p = pred.copy()  # a value >= n
    p[i, j] = n
    cases.append((p, "range"))
    p = pred.copy()  # a pair that is not a link
    p[i, j] = non_link(j, ())
    cases.append((p, "link"))
    for p, word in cases:
        want = PR.first_bad_pred(g, nodes, (0, n), p, ri, cj)
        assert want is not None and want[0] == i
        rc, pair, msg = run(p)
        assert rc == _capi.SG_ERR_INVALID_ARG and pair == want and word in msg, (word, pair, want, msg)
    # without out_link no link is looked up: the non-link is not reported
    assert PR.first_bad_pred(g, nodes, (0, n), cases[2][0], ri, cj, links=False) is None
    assert run(cases[2][0], ("node", "lat", "loss"))[0] == _capi.SG_OK
    # precedence: a non-link in an earlier row, a value >= n in a later one
    later = int(np.flatnonzero((ri > i) & (ri != cj))[0])
    p = cases[2][0].copy()
    p[int(ri[later]), int(cj[later])] = n + 5
    want = PR.first_bad_pred(g, nodes, (0, n), p, ri, cj)
    assert want == (int(ri[later]), int(cj[later])) and want > PR.first_bad_pred(g, nodes, (0, n), cases[2][0], ri, cj)
    rc, pair, msg = run(p)
    assert rc == _capi.SG_ERR_INVALID_ARG and pair == want and "range" in msg, (pair, want, msg)
    # the same corruption in a cell no path crosses succeeds
    crossed = np.zeros(n, bool)
    for c in cj[ri == i].tolist():
        if c != i:
            crossed[above(i, c)] = True
    free = int(np.flatnonzero(~crossed)[0])
    assert free != i
    for bad in (n, next(x for x in range(n) if x != free and LR.link_index(keys, [x], [free])[0] < 0)):
        p = pred.copy()
        p[i, free] = bad
        assert PR.first_bad_pred(g, nodes, (0, n), p, ri, cj) is None
        assert run(p)[0] == _capi.SG_OK
    # and the context still works
    _check(net, nodes, (0, n), tie["tabs"], _want_packets(tie, hosts, pk, None), ht=tie["ht"], pb=pb)


def test_item_and_argument_errors(ctx, tie):
    """(k): packet and pair errors report their index; host-side argument errors leave every
    output, out_off and *total included, as it was."""
    from shadow_amd import _capi

    g, net, nodes, hosts, ht = tie["g"], tie["net"], tie["nodes"], tie["hosts"], tie["ht"]
    n = g["n"]
    pred, lat, loss = tie["tabs"]
    base = {k: v[:2000].copy() for k, v in tie["pk"].items()}
    st = np.zeros(2000, np.uint8)
    st[700] = RC.DROP_NO_DST

    def run(pk, status, r0=0, r1=n):
        outs = _sentinels(2000, 30000)
        rc, _ = _call(net, nodes, r0, r1, (pred[r0:r1], lat[r0:r1], loss[r0:r1]), outs, 30000, ht=ht, pb=_batch(pk),
                      status=_dev(status, np.uint8))
        return (rc,) + _error(ctx)

    # a source host out of range
    pk = dict(base, src=base["src"].copy())
    pk["src"][1234] = hosts["n"]
    rc, pair, msg = run(pk, st)
    assert rc == _capi.SG_ERR_INVALID_ARG and pair == (1234, UMAX) and "source host" in msg, (pair, msg)
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
    assert run(pk, None)[1] == (700, UMAX)
    # the pair form: a row outside the block, a column >= n
    ri, cj = PC.tie_pairs(257)
    in40 = ri % 40
    in40[[77, 200]] = 45
    for bad_r, bad_c, r1, word in ((in40, cj, 40, "row"), (ri, np.where(np.arange(257) % 100 == 30, n, cj), n, "column")):
        want = PR.first_bad_pair((0, r1), n, bad_r, bad_c)
        assert want is not None and want > 0
        outs = _sentinels(257, 4000)
        rc, _ = _call(net, nodes, 0, r1, (pred[:r1], lat[:r1], loss[:r1]), outs, 4000, pairs=(bad_r, bad_c), dev=True)
        pair, msg = _error(ctx)
        assert rc == _capi.SG_ERR_INVALID_ARG and pair == (want, UMAX) and word in msg, (pair, want, msg)
    # host-side argument errors
    outs = _sentinels(2000, 30000)
    pb = _batch(base)
    dup = nodes.copy()
    dup[5] = 6
    other = _net(LC.multi_graph(), ctx)
    tabs = (pred, lat, loss)
    kw = dict(ht=ht, pb=pb)
    codes = [_call(net, dup, 0, n, tabs, outs, 30000, **kw),
             _call(net, nodes[:40], 0, 4, tabs, outs, 30000, **kw),
             _call(net, nodes, 3, 2, tabs, outs, 30000, **kw),
             _call(net, nodes, n - 1, n + 1, tabs, outs, 30000, **kw),
             _call(other, nodes, 0, n, tabs, outs, 30000, **kw),
             _call(net, nodes, 0, n, (None, lat, loss), outs, 30000, **kw),
             _call(net, nodes, 0, n, (pred, None, loss), outs, 30000, **kw),  # out_latency_ns without its rows
             _call(net, nodes, 0, n, (pred, lat, None), outs, 30000, **kw),  # out_packet_loss without its rows
             _call(net, nodes, 0, n, tabs, dict(outs, node=None, link=None, lat=None, loss=None), 30000, **kw),
             _call(net, nodes, 0, n, tabs, dict(outs, off=None), 30000, **kw),
             _call(net, nodes, 0, n, tabs, dict(outs, node=None, link=None, lat=None, loss=None), 0, pairs=(ri, cj))]
    assert [c for c, _ in codes] == [_capi.SG_ERR_INVALID_ARG] * len(codes)
    assert all(t == 0xDEAD for _, t in codes)
    L, h, nh, p = _capi.load(), ctx.handle, net._ensure_net(), pb.c_struct()
    a = [outs[k].ctypes.data for k in ("off",) + NAMES]
    B, Ns, T = _capi.C.byref(p), nodes.ctypes.data, _capi.C.byref(_capi.C.c_uint64())
    P, Tl, Tf = pred.ctypes.data, lat.ctypes.data, loss.ctypes.data
    bad = [L.sg_tree_paths_packets(h, None, ht.handle, Ns, n, 0, n, 0, P, Tl, Tf, B, None, *a, 30000, T),
           L.sg_tree_paths_packets(h, nh, None, Ns, n, 0, n, 0, P, Tl, Tf, B, None, *a, 30000, T),
           L.sg_tree_paths_packets(h, nh, ht.handle, None, n, 0, n, 0, P, Tl, Tf, B, None, *a, 30000, T),
           L.sg_tree_paths_packets(h, nh, ht.handle, Ns, n, 0, n, 0, P, Tl, Tf, None, None, *a, 30000, T),
           L.sg_tree_paths_packets(h, nh, ht.handle, Ns, n, 0, n, 0, P, Tl, Tf, B, None, *a, 30000, None),
           L.sg_tree_paths(h, None, Ns, n, 0, n, 0, P, Tl, Tf, 257, ri.ctypes.data, cj.ctypes.data, *a, 30000, T),
           L.sg_tree_paths(h, nh, Ns, n, 0, n, 0, P, Tl, Tf, 257, ri.ctypes.data, None, *a, 30000, T)]
    assert bad == [_capi.SG_ERR_INVALID_ARG] * len(bad)
    assert _untouched(outs)


def test_host_arrays_pair_form(ctx, tie):
    """(l): the pair form on host arrays, no pairs at all included."""
    from shadow_amd import _capi

    ri, cj = PC.tie_pairs(257)
    want = PR.records(tie["g"], tie["nodes"], (0, 300), tie["tabs"][0], tie["olat"], tie["oloss"], ri.astype(np.int64), cj)
    _check(tie["net"], tie["nodes"], (0, 300), tie["tabs"], want, pairs=(ri, cj))
    for dev in (False, True):
        outs = _sentinels(0, PAD)
        rc, total = _call(tie["net"], tie["nodes"], 0, 300, tie["tabs"], outs, PAD, pairs=(ri[:0], cj[:0]), dev=dev)
        assert rc == _capi.SG_OK and total == 0 and outs["off"].tolist() == [0]
        assert _untouched(dict(outs, off=np.full(1, PC.SENT_OFF, np.uint64)))


def test_python_interface(ctx, tie):
    """(m): PathTree.paths against PathTree.path on 200 pairs; PathTree.trace_round."""
    g, net, hosts, pk = tie["g"], tie["net"], tie["hosts"], tie["pk"]
    t = net.compute_shortest_path_tree()
    rng = np.random.default_rng(71)
    src, dst = rng.integers(0, 300, 200), rng.integers(0, 300, 200)
    dst[:3] = src[:3]
    off, node, link, lat, loss = t.paths(src, dst)
    assert off.dtype == np.uint64 and node.dtype == link.dtype == np.uint32 and lat.dtype == np.uint64
    assert loss.dtype == np.float32 and len(off) == 201 and len(node) == len(link) == len(lat) == len(loss) == int(off[-1])
    tail, head = net.links()
    for p in range(200):
        a, b = int(off[p]), int(off[p + 1])
        s, d = int(src[p]), int(dst[p])
        if s == d:
            assert node[a:b].tolist() == [s] and t.path(s, d) == [s]
        else:
            assert [s] + node[a:b].tolist() == t.path(s, d)
        assert tail[link[a:b]].tolist() == ([s] + node[a:b].tolist())[:-1] and head[link[a:b]].tolist() == node[a:b].tolist()
        cols = [t.index[v] for v in node[a:b].tolist()]
        assert np.array_equal(lat[a:b], t.latency_ns[t.index[s], cols])
        assert np.array_equal(loss[a:b].view(np.uint32), t.packet_loss[t.index[s], cols].view(np.uint32))
    with pytest.raises(ValueError):
        t.paths([1, 2], [3])
    st = RC.mixed_status(len(pk["src"]))
    want = PR.packet_records(g, t.nodes, (0, 300), t.pred, tie["olat"], tie["oloss"], hosts, pk, st)
    got = t.trace_round(tie["ht"], tie["pb"], st)
    for a, w in zip(got, want):
        assert a.dtype == w.dtype and np.array_equal(a.view(np.uint8), w.view(np.uint8))
    got = t.trace_round(tie["ht"], tie["pb"])
    want = PR.packet_records(g, t.nodes, (0, 300), t.pred, tie["olat"], tie["oloss"], hosts, pk, None)
    for a, w in zip(got, want):
        assert np.array_equal(a.view(np.uint8), w.view(np.uint8))
    # more records than the first call's guess: the second call at the reported total
    gp = LC.path_graph(4096)
    tp = _net(gp, ctx).compute_shortest_path_tree([0])
    off, node, link, lat, _ = tp.paths([0, 0, 0], [4095, 1, 0])
    assert off.tolist() == [0, 4095, 4096, 4097] and len(node) == len(link) == 4097
    assert [0] + node[:4095].tolist() == tp.path(0, 4095) and node[4095:].tolist() == [1, 0]
    assert np.array_equal(lat[:4095], tp.latency_ns[0, [tp.index[v] for v in node[:4095].tolist()]])
