"""The link trace on the GPU (sg_link_trace_packets, NetworkGraph.link_trace_packets_device,
PathTree.link_trace_round).

In every case the pred and latency rows the library reads come from sg_routing_build_tree on the
same net: their own correctness is test_tree_gpu.py's, here they are inputs.  The reference
(tests/trace_ref.py) transposes the hop records of tests/paths_ref.py, with latencies from the
oracle's table, and sorts them with one lexsort.  Every output starts from sentinels, a few records
longer than the total, so that "nothing past the total is written" is itself checked; every
comparison is exact (np.array_equal).  The inputs' own conditions are checked on the CPU in
test_trace_ref_cpu.py."""
import itertools

import numpy as np
import pytest

import link_cases as LC
import link_ref as LR
import link_round_cases as RC
import link_round_ref as RR
import paths_ref as PR
import sweep_cases as SC
import trace_cases as XC
import trace_ref as XR
from shadow_amd import synth

pytestmark = pytest.mark.gpu

UMAX = 0xFFFFFFFF
PAD = 3  # sentinel records past the total
NAMES = ("packet", "hop", "enter", "exit")
KEYS = ("off",) + NAMES
VIEW = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def _net(g, ctx):
    from shadow_amd import NetworkGraph

    return NetworkGraph(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], ctx=ctx)


def _tabs(net, nodes, r0, r1):
    """(pred, latency) rows [r0, r1) from sg_routing_build_tree (host outputs)."""
    from shadow_amd import _capi

    nodes = np.ascontiguousarray(nodes, np.uint32)
    n, k = len(nodes), r1 - r0
    lat, loss = np.zeros((k, n), np.uint64), np.zeros((k, n), np.float32)
    pred, hop = np.zeros((k, n), np.uint32), np.zeros((k, n), np.uint32)
    _capi.check(net.ctx.handle, _capi.load().sg_routing_build_tree(
        net.ctx.handle, net._ensure_net(), nodes.ctypes.data, n, r0, r1, _capi.SG_ROUTE_SHORTEST_PATH,
        lat.ctypes.data, loss.ctypes.data, pred.ctypes.data, hop.ctypes.data))
    return pred, lat


def _oracle_lat(O, g, nodes, r0, r1):
    rc, lat, _, _ = O.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"],
                                     np.asarray(nodes, np.uint32), rows=(r0, r1), threads=8)
    assert rc == 0
    return lat


def _host_table(hosts, ctx):
    from shadow_amd.worker import HostTable

    return HostTable(hosts["ip"], hosts["route"], hosts["seed"], ctx=ctx)


def _batch(pk):
    from shadow_amd.worker import PacketBatch

    n = len(pk["src"])
    return PacketBatch.from_numpy(pk["src"], pk["dst_ip"], pk.get("payload", np.zeros(n, np.uint32)), pk["send_time"])


def _dev(x):
    import torch

    if x is None:
        return None
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(VIEW[x.dtype]).copy()).cuda()


def _sentinels(n_links, cap, which=NAMES):
    outs = dict(off=np.full(n_links + 1, XC.SENT_OFF, np.uint64), packet=np.full(cap, XC.SENT32, np.uint32),
                hop=np.full(cap, XC.SENT32, np.uint32), enter=np.full(cap, XC.SENT64, np.uint64),
                exit=np.full(cap, XC.SENT64, np.uint64))
    for k in NAMES:
        if k not in which:
            outs[k] = None
    return outs


def _untouched(outs, off=True):
    want = _sentinels(len(outs["off"]) - 1, max(len(v) for k, v in outs.items() if k != "off" and v is not None))
    return all(v is None or (k == "off" and not off) or np.array_equal(v, want[k]) for k, v in outs.items())


def _call(net, nodes, r0, r1, tabs, outs, cap, ht, pb, status=None, watch=None, dev=False, n_nodes=None):
    """One call on numpy arrays: host-array mode, or (dev) everything uploaded, SG_ROUTE_OUT_DEVICE,
    and the outputs copied back into `outs`.  tabs = (pred or None, latency or None); status: a
    numpy u8 array or None; watch: a numpy u8 mask or None.  Returns (status code, total)."""
    import torch

    from shadow_amd import _capi

    C = _capi.C
    nodes = np.ascontiguousarray(nodes, np.uint32)
    ins = [None if t is None else np.ascontiguousarray(t, dt) for t, dt in zip(tabs, (np.uint32, np.uint64))]
    ins.append(None if watch is None else np.ascontiguousarray(watch, np.uint8))
    d_status = _dev(status)
    if dev:
        d_ins = [_dev(t) for t in ins]
        d_outs = {k: _dev(outs[k]) for k in KEYS}
        ip = [None if t is None else C.c_void_p(t.data_ptr()) for t in d_ins]
        op = [None if d_outs[k] is None else C.c_void_p(d_outs[k].data_ptr()) for k in KEYS]
    else:
        ip = [None if t is None else t.ctypes.data for t in ins]
        op = [None if outs[k] is None else outs[k].ctypes.data for k in KEYS]
    total = C.c_uint64(0xDEAD)
    p = pb.c_struct()
    rc = _capi.load().sg_link_trace_packets(
        net.ctx.handle, net._ensure_net(), ht.handle, nodes.ctypes.data, len(nodes) if n_nodes is None else n_nodes, r0, r1,
        _capi.SG_ROUTE_OUT_DEVICE if dev else 0, ip[0], ip[1], C.byref(p),
        None if d_status is None else C.c_void_p(d_status.data_ptr()), ip[2], *op, cap, C.byref(total))
    if dev:
        torch.cuda.synchronize()
        for k in KEYS:
            if outs[k] is not None:
                outs[k][...] = d_outs[k].cpu().numpy().view(outs[k].dtype)
    return rc, total.value


def _error(ctx):
    from shadow_amd import _capi

    r, k = _capi.C.c_uint32(), _capi.C.c_uint32()
    _capi.load().sg_ctx_last_error_pair(ctx.handle, _capi.C.byref(r), _capi.C.byref(k))
    return (r.value, k.value), _capi.load().sg_ctx_last_error(ctx.handle).decode()


def _same(outs, want, which=NAMES):
    """The outputs against the reference (off, packet, hop, enter, exit); the tail still sentinels."""
    off, total = want[0], int(want[0][-1])
    assert np.array_equal(outs["off"], off), f"offsets differ at {int((outs['off'] != off).sum())} entries"
    tail = _sentinels(0, PAD)
    for k, w in zip(NAMES, want[1:]):
        if k not in which:
            continue
        got = outs[k]
        assert np.array_equal(got[:total], w), f"{k} differs at {int((got[:total] != w).sum())} of {total} records"
        assert np.array_equal(got[total:], tail[k][:len(got) - total]), f"{k}: written past the total"


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
    """The tie graph's net, its rows from the library and the oracle's latencies, (a)'s hosts and batch."""
    g = LC.tie_graph()
    nodes = np.arange(g["n"], dtype=np.uint32)
    net = _net(g, ctx)
    hosts, pk, mixed = XC.tie_round()
    tabs = _tabs(net, nodes, 0, g["n"])
    olat = _oracle_lat(oracle, g, nodes, 0, g["n"])
    assert np.array_equal(tabs[1], olat)
    return dict(g=g, nodes=nodes, net=net, tabs=tabs, olat=olat, hosts=hosts, pk=pk, mixed=mixed,
                ht=_host_table(hosts, ctx), pb=_batch(pk), n_links=XR.n_links(g))


def _want(t, hosts, pk, status=None, watch=None):
    return XR.trace(t["g"], t["nodes"], (0, 300), t["tabs"][0], t["olat"], hosts, pk, status, watch)


def _head(pk, n):
    return {k: v[:n] for k, v in pk.items()}


@pytest.mark.parametrize("dev", [True, False], ids=["device", "host"])
def test_tie_round(ctx, tie, dev):
    """(a): 10,000 packets whose every key ties in its time with another's; mixed statuses, and
    status = NULL.  The timers count the records."""
    for status in (tie["mixed"], None):
        want = _want(tie, tie["hosts"], tie["pk"], status)
        ctx.enable_timers(True)
        try:
            _check(tie["net"], tie["nodes"], (0, 300), tie["tabs"], want, ht=tie["ht"], pb=tie["pb"], status=status, dev=dev)
            for name in ("link_trace_count", "link_trace_fill", "link_trace_sort"):
                _, launches, work = ctx.read_timer(name)
                assert launches == 1 and int(work) == int(want[0][-1]), (name, launches, work)
        finally:
            ctx.enable_timers(False)


@pytest.mark.parametrize("shuffled", [False, True], ids=["one_time", "shuffled_times"])
def test_tiers(ctx, oracle, monkeypatch, shuffled):
    """(b): segments of 1 .. 3 P - 1 records on two links: the wave's rank sort, the LDS sort of
    one piece, the merge of two and of three pieces; P = 128 by the test knob, and the three
    longest at the default P."""
    g = XC.tier_graph()
    net = _net(g, ctx)
    nodes = np.arange(3, dtype=np.uint32)
    tabs = _tabs(net, nodes, 0, 1)
    olat = _oracle_lat(oracle, g, nodes, 0, 1)
    for piece, lengths in ((XC.PIECE, XC.tier_lengths(XC.PIECE)), (None, XC.tier_lengths(XC.PIECE_DEFAULT)[-3:])):
        if piece is None:
            monkeypatch.delenv("SG_LINK_TRACE_PIECE")
        else:
            monkeypatch.setenv("SG_LINK_TRACE_PIECE", str(piece))
        for n in lengths:
            hosts, pk = XC.tier_round(n, shuffled)
            want = XR.trace(g, nodes, (0, 1), tabs[0], olat, hosts, pk)
            assert int(want[0][-1]) == 2 * n
            _check(net, nodes, (0, 1), tabs, want, ht=_host_table(hosts, ctx), pb=_batch(pk), dev=True)


def test_output_subsets(ctx, tie):
    """(c): each record output alone, and every subset that leaves one out."""
    pk = _head(tie["pk"], 3000)
    want = _want(tie, tie["hosts"], pk)
    pb = _batch(pk)
    for which in list(itertools.combinations(NAMES, 1)) + list(itertools.combinations(NAMES, 3)):
        _check(tie["net"], tie["nodes"], (0, 300), tie["tabs"], want, which, ht=tie["ht"], pb=pb)
        _check(tie["net"], tie["nodes"], (0, 300), tie["tabs"], want, which, ht=tie["ht"], pb=pb, dev=True)


def test_watch(ctx, tie):
    """(d): no link watched (total 0, equal offsets, no record written); one link; every other
    link; a crossing that is not a link is reported though nothing is watched."""
    from shadow_amd import _capi

    net, nodes, tabs, nl = tie["net"], tie["nodes"], tie["tabs"], tie["n_links"]
    pk = _head(tie["pk"], 4000)
    pb = _batch(pk)
    every = _want(tie, tie["hosts"], pk)
    busiest = int(np.argmax(np.diff(every[0].astype(np.int64))))
    masks = [np.zeros(nl, np.uint8), (np.arange(nl) == busiest).astype(np.uint8), (np.arange(nl) % 2).astype(np.uint8)]
    for dev in (False, True):
        for m in masks:
            want = _want(tie, tie["hosts"], pk, None, m)
            outs = _check(net, nodes, (0, 300), tabs, want, ht=tie["ht"], pb=pb, watch=m, dev=dev)
            if not m.any():
                assert not outs["off"].any() and _untouched(outs, off=False)
        want = _want(tie, tie["hosts"], pk, None, masks[1])
        assert int(want[0][-1]) == int(np.diff(every[0].astype(np.int64)).max()) > 0
    # a walked (pred, node) pair that is not a link, no link watched
    pred = tabs[0]
    _, _, keys = LR.links(tie["g"])
    _, ri, cj = RR.counted_pairs(tie["hosts"], pk, None)
    k = int(np.flatnonzero((ri != cj) & (pred[ri, cj] != ri))[0])
    i, j = int(ri[k]), int(cj[k])
    p = pred.copy()
    p[i, j] = next(x for x in range(300) if x != j and LR.link_index(keys, [x], [j])[0] < 0)
    want = PR.first_bad_pred(tie["g"], nodes, (0, 300), p, ri, cj)
    assert want is not None and want[0] == i
    outs = _sentinels(nl, 100)
    rc, _ = _call(net, nodes, 0, 300, (p, tabs[1]), outs, 100, ht=tie["ht"], pb=pb, watch=masks[0])
    pair, msg = _error(ctx)
    assert rc == _capi.SG_ERR_INVALID_ARG and pair == want and "link" in msg, (pair, want, msg)


def test_shuffled_nodes_two_row_blocks(ctx, tie, oracle):
    """(e): a shuffled node order; each row block's call with its own pred and latency blocks."""
    g, net = tie["g"], tie["net"]
    nodes, hosts, lo, hi = RC.shuffled_round()
    ht = _host_table(hosts, ctx)
    for (r0, r1), pk in (((0, 60), lo), ((60, 120), hi)):
        tabs = _tabs(net, nodes, r0, r1)
        want = XR.trace(g, nodes, (r0, r1), tabs[0], _oracle_lat(oracle, g, nodes, r0, r1), hosts, pk)
        _check(net, nodes, (r0, r1), tabs, want, ht=ht, pb=_batch(pk))
        _check(net, nodes, (r0, r1), tabs, want, ht=ht, pb=_batch(pk), dev=True)


@pytest.mark.parametrize("which", ["directed", "multi"])
def test_directed_and_multigraph(ctx, oracle, which):
    """(e): packets to the sender's own node give self-loop records carrying the diagonal cell;
    a general batch beside them; parallel edges are one link."""
    g = LC.directed_graph() if which == "directed" else LC.multi_graph()
    n = g["n"]
    net = _net(g, ctx)
    nodes = np.arange(n, dtype=np.uint32)
    tabs = _tabs(net, nodes, 0, n)
    olat = _oracle_lat(oracle, g, nodes, 0, n)
    hosts, pk = RC.same_node_round(n)
    ht = _host_table(hosts, ctx)
    want = XR.trace(g, nodes, (0, n), tabs[0], olat, hosts, pk)
    outs = _check(net, nodes, (0, n), tabs, want, ht=ht, pb=_batch(pk))
    tail, head = net.links()
    loops = np.flatnonzero(tail == head)
    assert len(loops) == n and np.array_equal(np.diff(outs["off"].astype(np.int64)), 2 * (tail == head))
    node = np.repeat(tail[loops], 2).astype(np.int64)
    assert (outs["hop"][:2 * n] == 1).all() and (outs["enter"][:2 * n] == RC.T0).all()
    assert np.array_equal(outs["exit"][:2 * n], np.uint64(RC.T0) + olat[node, node])
    assert np.array_equal(hosts["route"][pk["src"][outs["packet"][:2 * n]]], node)
    pk2 = RC.batch(3000, hosts, 47)
    want = XR.trace(g, nodes, (0, n), tabs[0], olat, hosts, pk2)
    _check(net, nodes, (0, n), tabs, want, ht=ht, pb=_batch(pk2), dev=True)


def test_sparse_addresses(ctx, tie):
    """(e): the sorted address table resolves; packets to unknown addresses have no record."""
    hosts, pk, status = RC.sparse_address_round()
    want = _want(tie, hosts, pk, status)
    _check(tie["net"], tie["nodes"], (0, 300), tie["tabs"], want, ht=_host_table(hosts, ctx), pb=_batch(pk), status=status)


def test_wide_cells_and_overflow(ctx, oracle):
    """(f): latencies past 2^32 ns and enter times on both sides of 2^32 inside a segment; a
    counted packet whose arrival passes 2^64 - 1 is SG_ERR_TIME_OVERFLOW with its index, the
    smallest such; one at 2^64 - 1 exactly is not; the same packet not counted is no error."""
    from shadow_amd import _capi

    g = XC.wide_graph()
    n = g["n"]
    net = _net(g, ctx)
    nodes = np.arange(n, dtype=np.uint32)
    tabs = _tabs(net, nodes, 0, n)
    olat = _oracle_lat(oracle, g, nodes, 0, n)
    assert np.array_equal(tabs[1], olat)
    hosts, pk = XC.wide_round()
    ht = _host_table(hosts, ctx)
    want = XR.trace(g, nodes, (0, n), tabs[0], olat, hosts, pk)
    for dev in (False, True):
        _check(net, nodes, (0, n), tabs, want, ht=ht, pb=_batch(pk), dev=dev)
    _, ri, cj = RR.counted_pairs(hosts, pk, None)
    cell = olat[ri, cj].astype(object)
    late = dict(pk, send_time=pk["send_time"].copy())
    late["send_time"][700] = np.uint64((1 << 64) - 1 - int(cell[700]))  # arrives at 2^64 - 1
    want = XR.trace(g, nodes, (0, n), tabs[0], olat, hosts, late)
    assert XR.first_overflow(nodes, (0, n), olat, hosts, late) is None and int(want[4].max()) == (1 << 64) - 1
    _check(net, nodes, (0, n), tabs, want, ht=ht, pb=_batch(late), dev=True)
    for q in (2000, 1300):
        late["send_time"][q] = np.uint64((1 << 64) - int(cell[q]))  # one past it
    for status, first in ((None, 1300), (np.where(np.arange(len(ri)) == 1300, RC.DROP_LOSS, 0).astype(np.uint8), 2000)):
        assert XR.first_overflow(nodes, (0, n), olat, hosts, late, status) == first
        outs = _sentinels(len(want[0]) - 1, 40000)
        rc, _ = _call(net, nodes, 0, n, tabs, outs, 40000, ht=ht, pb=_batch(late), status=status, dev=True)
        pair, msg = _error(ctx)
        assert rc == _capi.SG_ERR_TIME_OVERFLOW and pair == (first, UMAX) and f"packet {first} " in msg, (rc, pair, msg)
    status = np.where(np.isin(np.arange(len(ri)), (1300, 2000)), RC.SIM_END, 0).astype(np.uint8)
    assert XR.first_overflow(nodes, (0, n), olat, hosts, late, status) is None
    want = XR.trace(g, nodes, (0, n), tabs[0], olat, hosts, late, status)
    _check(net, nodes, (0, n), tabs, want, ht=ht, pb=_batch(late), status=status, dev=True)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_capacity(ctx, tie, dev):
    """(g): cap one below the total: SG_ERR_CAPACITY, out_link_off and *total complete, no
    record written; the second call at cap = total succeeds."""
    from shadow_amd import _capi

    pk = _head(tie["pk"], 2000)
    pb = _batch(pk)
    want = _want(tie, tie["hosts"], pk)
    total = int(want[0][-1])
    outs = _sentinels(tie["n_links"], total + PAD)
    rc, got = _call(tie["net"], tie["nodes"], 0, 300, tie["tabs"], outs, total - 1, ht=tie["ht"], pb=pb, dev=dev)
    assert rc == _capi.SG_ERR_CAPACITY and got == total
    assert np.array_equal(outs["off"], want[0]) and _untouched(outs, off=False)
    rc, got = _call(tie["net"], tie["nodes"], 0, 300, tie["tabs"], outs, total, ht=tie["ht"], pb=pb, dev=dev)
    assert rc == _capi.SG_OK and got == total
    _same(outs, want)


def test_corrupted_pred(ctx, tie):
    """(h): a 2-cycle, a value >= n and a non-link on a walked path, each with its (row, col); a
    value >= n comes ahead of a non-link with a smaller (row, col); the same corruption in an
    unwalked cell succeeds."""
    from shadow_amd import _capi

    g, net, nodes, hosts = tie["g"], tie["net"], tie["nodes"], tie["hosts"]
    n = g["n"]
    pred, lat = tie["tabs"]
    pk = _head(tie["pk"], 3000)
    pb = _batch(pk)
    _, _, keys = LR.links(g)
    _, ri, cj = RR.counted_pairs(hosts, pk, None)
    # a walked cell: the destination of the first packet with two hops or more
    k = int(np.flatnonzero((ri != cj) & (pred[ri, cj] != ri))[0])
    i, j = int(ri[k]), int(cj[k])

    def run(p, which=NAMES):
        outs = _sentinels(tie["n_links"], 40000, which)
        rc, _ = _call(net, nodes, 0, n, (p, lat), outs, 40000, ht=tie["ht"], pb=pb)
        return (rc,) + _error(ctx)

    def above(row, x):  # the nodes from x up to the row's source
        seen = [x]
        while seen[-1] != row:
            seen.append(int(pred[row, seen[-1]]))
        return seen

    cases = []
    p = pred.copy()  # a 2-cycle on that packet's path
    p[i, int(p[i, j])] = j
    cases.append((p, "cycle"))
    p = pred.copy()  # a value >= n
    p[i, j] = n
    cases.append((p, "range"))
    p = pred.copy()  # a pair that is not a link
    p[i, j] = next(x for x in range(n) if x != j and LR.link_index(keys, [x], [j])[0] < 0 and j not in above(i, x))
    cases.append((p, "link"))
    for p, word in cases:
        want = PR.first_bad_pred(g, nodes, (0, n), p, ri, cj)
        assert want is not None and want[0] == i
        rc, pair, msg = run(p)
        assert rc == _capi.SG_ERR_INVALID_ARG and pair == want and word in msg, (word, pair, want, msg)
    # every crossing is looked up: the non-link is reported whichever outputs are asked for
    rc, pair, _ = run(cases[2][0], ("enter",))
    assert rc == _capi.SG_ERR_INVALID_ARG and pair == PR.first_bad_pred(g, nodes, (0, n), cases[2][0], ri, cj)
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
    _check(net, nodes, (0, n), tie["tabs"], _want(tie, hosts, pk), ht=tie["ht"], pb=pb)


def test_packet_and_argument_errors(ctx, tie):
    """(h): packet errors report their index; host-side argument errors leave every output,
    out_link_off and *total included, as it was."""
    from shadow_amd import _capi

    g, net, nodes, hosts, ht = tie["g"], tie["net"], tie["nodes"], tie["hosts"], tie["ht"]
    n, nl = g["n"], tie["n_links"]
    pred, lat = tie["tabs"]
    base = {k: v[:2000].copy() for k, v in tie["pk"].items()}
    st = np.zeros(2000, np.uint8)
    st[700] = RC.DROP_NO_DST

    def run(pk, status, r0=0, r1=n):
        outs = _sentinels(nl, 30000)
        rc, _ = _call(net, nodes, r0, r1, (pred[r0:r1], lat[r0:r1]), outs, 30000, ht=ht, pb=_batch(pk), status=status)
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
    # host-side argument errors
    outs = _sentinels(nl, 30000)
    pb = _batch(base)
    dup = nodes.copy()
    dup[5] = 6
    other = _net(LC.multi_graph(), ctx)
    tabs = (pred, lat)
    kw = dict(ht=ht, pb=pb)
    none = dict(outs, packet=None, hop=None, enter=None, exit=None)
    codes = [_call(net, dup, 0, n, tabs, outs, 30000, **kw),
             _call(net, nodes[:40], 0, 4, tabs, outs, 30000, **kw),
             _call(net, nodes, 3, 2, tabs, outs, 30000, **kw),
             _call(net, nodes, n - 1, n + 1, tabs, outs, 30000, **kw),
             _call(other, nodes, 0, n, tabs, outs, 30000, **kw),
             _call(net, nodes, 0, n, (None, lat), outs, 30000, **kw),
             _call(net, nodes, 0, n, (pred, None), outs, 30000, **kw),  # the order needs the latency rows
             _call(net, nodes, 0, n, tabs, none, 30000, **kw),
             _call(net, nodes, 0, n, tabs, none, 0, **kw),  # a sizing call passes a real record array
             _call(net, nodes, 0, n, tabs, dict(outs, off=None), 30000, **kw)]
    assert [c for c, _ in codes] == [_capi.SG_ERR_INVALID_ARG] * len(codes)
    assert all(t == 0xDEAD for _, t in codes)
    L, h, nh, p = _capi.load(), ctx.handle, net._ensure_net(), pb.c_struct()
    a = [outs[k].ctypes.data for k in KEYS]
    B, Ns, T = _capi.C.byref(p), nodes.ctypes.data, _capi.C.byref(_capi.C.c_uint64())
    P, Tl = pred.ctypes.data, lat.ctypes.data
    no_time = pb.c_struct()
    no_time.send_time_ns = None
    bad = [L.sg_link_trace_packets(h, None, ht.handle, Ns, n, 0, n, 0, P, Tl, B, None, None, *a, 30000, T),
           L.sg_link_trace_packets(h, nh, None, Ns, n, 0, n, 0, P, Tl, B, None, None, *a, 30000, T),
           L.sg_link_trace_packets(h, nh, ht.handle, None, n, 0, n, 0, P, Tl, B, None, None, *a, 30000, T),
           L.sg_link_trace_packets(h, nh, ht.handle, Ns, n, 0, n, 0, P, Tl, None, None, None, *a, 30000, T),
           L.sg_link_trace_packets(h, nh, ht.handle, Ns, n, 0, n, 0, P, Tl, _capi.C.byref(no_time), None, None, *a, 30000, T),
           L.sg_link_trace_packets(h, nh, ht.handle, Ns, n, 0, n, 0, P, Tl, B, None, None, *a, 30000, None)]
    assert bad == [_capi.SG_ERR_INVALID_ARG] * len(bad)
    assert _untouched(outs)
    # no packets at all: every offset zero, no record
    for dev in (False, True):
        outs = _sentinels(nl, PAD)
        rc, total = _call(net, nodes, 0, n, tabs, outs, PAD, ht=ht, pb=_batch(_head(base, 0)), dev=dev)
        assert rc == _capi.SG_OK and total == 0 and not outs["off"].any() and _untouched(outs, off=False)


def test_star_hot_link(ctx, oracle):
    """(i): the 512-spoke star, 3,000 packets from one spoke: its link to the hub holds nearly
    all of them (the merge tier at the default piece), 500 and more links one or two."""
    g = LC.star_graph(512)
    net = _net(g, ctx)
    nodes = np.arange(g["n"], dtype=np.uint32)
    hosts, pk = RC.star_round()
    tabs = _tabs(net, nodes, 0, 8)
    want = XR.trace(g, nodes, (0, 8), tabs[0], _oracle_lat(oracle, g, nodes, 0, 8), hosts, pk)
    cnt = np.diff(want[0].astype(np.int64))
    assert int(cnt.max()) > XC.PIECE_DEFAULT and int((cnt > 0).sum()) >= 500 and int(np.sort(cnt)[-2]) <= 64
    for dev in (False, True):
        _check(net, nodes, (0, 8), tabs, want, ht=_host_table(hosts, ctx), pb=_batch(pk), dev=dev)


def test_c3_shape(ctx):
    """(j): rows [0, 512) of the C3 shape, 50,000 packets to hosts anywhere: the records per link
    are sg_link_load_packets' loads, (packet, hop) finds the segment's own link in
    sg_tree_paths_packets' records, the times are the send time plus those records' latencies,
    and every segment ascends in (enter, packet)."""
    import torch

    g = LC.c3_graph()
    net = _net(g, ctx)
    nodes = np.arange(10000, dtype=np.uint32)
    hosts, pk = RC.c3_round()
    ht, pb = _host_table(hosts, ctx), _batch(pk)
    pred, lat = _tabs(net, nodes, 0, 512)
    dpred, dlat = _dev(pred), _dev(lat)
    nl, npk = len(net.links()[0]), len(pk["src"])
    cap = 16 * npk
    # the hop records and the loads
    doff = torch.zeros(npk + 1, dtype=torch.int64, device="cuda")
    dlink = torch.zeros(cap, dtype=torch.int32, device="cuda")
    dl = torch.zeros(cap, dtype=torch.int64, device="cuda")
    total = net.tree_paths_packets_device(ht, nodes, 0, 512, dpred.data_ptr(), dlat.data_ptr(), 0, pb, 0, doff.data_ptr(), 0,
                                          dlink.data_ptr(), dl.data_ptr(), 0, cap)
    assert 4 * npk < total <= cap
    dload = torch.zeros(nl, dtype=torch.int64, device="cuda")
    net.link_load_packets_device(ht, nodes, 0, 512, dpred.data_ptr(), pb, 0, 0, dload.data_ptr(), 0, 0)
    # the trace
    outs = {k: _dev(v) for k, v in _sentinels(nl, total + PAD).items()}
    rc, got = net.link_trace_packets_device(ht, nodes, 0, 512, dpred.data_ptr(), dlat.data_ptr(), pb, 0, 0,
                                            *[outs[k].data_ptr() for k in KEYS], total)
    torch.cuda.synchronize()
    assert rc == 0 and got == total
    off, packet, hop, enter, leave = (outs[k].cpu().numpy().view(dt) for k, dt in
                                      zip(KEYS, (np.uint64, np.uint32, np.uint32, np.uint64, np.uint64)))
    assert np.array_equal(np.diff(off.astype(np.int64)), dload.cpu().numpy()) and int(off[0]) == 0 and int(off[-1]) == total
    tail = _sentinels(0, PAD)
    for k, a in zip(NAMES, (packet, hop, enter, leave)):
        assert np.array_equal(a[total:], tail[k]), k
    packet, hop, enter, leave = packet[:total], hop[:total], enter[:total], leave[:total]
    poff, plink, plat = doff.cpu().numpy(), dlink.cpu().numpy().view(np.uint32), dl.cpu().numpy().view(np.uint64)
    at = poff[packet] + hop.astype(np.int64) - 1
    assert (hop >= 1).all() and (at < poff[packet.astype(np.int64) + 1]).all()
    seg = XR.segment_links(off)
    assert np.array_equal(plink[at].astype(np.int64), seg)
    send = pk["send_time"][packet]
    assert np.array_equal(leave, send + plat[at])
    assert np.array_equal(enter, send + np.where(hop > 1, plat[np.maximum(at - 1, 0)], np.uint64(0)))
    inside = seg[1:] == seg[:-1]
    ascends = (enter[1:] > enter[:-1]) | ((enter[1:] == enter[:-1]) & (packet[1:] > packet[:-1]))
    assert ascends[inside].all()


@pytest.mark.parametrize("n_links", sorted(XC.SCAN_EDGE))
def test_link_offsets_at_scan_tile_edges(ctx, n_links):
    """(m): one below, at and one past one scan tile (2,048) of link counters, the smallest sizes
    at which the scan's block boundary can go wrong for out_link_off: a path with 500 packets from
    sources spread along it.  The rows are the path's own (trace_cases.scan_edge_tables)."""
    assert SC.SCAN_TILE == 2048
    n, loops = XC.SCAN_EDGE[n_links]
    g = XC.scan_edge_graph(n, loops)
    assert len(LR.links(g)[0]) == n_links
    nodes, hosts, pk = XC.scan_edge_round(n)
    rows = (0, XC.SCAN_EDGE_ROWS)
    tabs = XC.scan_edge_tables(nodes)
    want = XR.trace(g, nodes, rows, tabs[0], tabs[1], hosts, pk)
    assert len(want[0]) == n_links + 1
    _check(_net(g, ctx), nodes, rows, tabs, want, ht=_host_table(hosts, ctx), pb=_batch(pk), dev=True)


@pytest.mark.parametrize("name", SC.NAMES)
def test_sweep(oracle, ctx, name):
    """(k): the 40 generated graphs, each row block's round with its mixed statuses."""
    c, rs = SC.case(name), SC.refs(oracle, name)
    net = _net(c["g"], ctx)
    ht = _host_table(c["hosts"], ctx)
    for v, r in zip(c["views"], rs):
        want = XR.trace(c["g"], c["nodes"], v["rows"], r["pred"], r["lat"], c["hosts"], v["pk"], v["status"])
        _check(net, c["nodes"], v["rows"], (r["pred"], r["lat"]), want, ht=ht, pb=_batch(v["pk"]), status=v["status"], dev=True)


def test_python_interface(ctx, tie):
    """(l): PathTree.link_trace_round from a round's Deliveries; watch as link numbers and as a
    mask; more records than the first call's guess."""
    import torch

    from shadow_amd.worker import DeviceTable, deliver_round

    g, net, nodes, hosts, pk = tie["g"], tie["net"], tie["nodes"], tie["hosts"], tie["pk"]
    t = net.compute_shortest_path_tree()
    assert np.array_equal(t.latency_ns, tie["olat"])
    dlat = torch.from_numpy(t.latency_ns.view(np.int64)).cuda()
    dloss = torch.from_numpy(t.packet_loss).cuda()
    # (a host table of its own: the round advances its hosts' streams)
    out = deliver_round(_host_table(hosts, ctx), DeviceTable(dlat.ravel(), dloss.ravel(), 300), tie["pb"], RC.ROUND_END,
                        2**63, 0, ctx=ctx)
    status = out.status[:len(pk["src"])].cpu().numpy()
    assert 0 < int((status == 0).sum()) == out.n_delivered < len(status)
    dtypes = (np.uint64, np.uint32, np.uint32, np.uint64, np.uint64)
    some = [5, 17, 400, 401, tie["n_links"] - 1]
    mask = np.zeros(tie["n_links"], bool)
    mask[some] = True
    for st, watch, ref_status in ((out, None, status), (status, some, status), (None, mask, None), (out, mask.astype(np.uint8), status)):
        got = t.link_trace_round(tie["ht"], tie["pb"], st, watch)
        want = XR.trace(g, t.nodes, (0, 300), t.pred, tie["olat"], hosts, pk, ref_status, None if watch is None else some)
        for a, w, dt in zip(got, want, dtypes):
            assert a.dtype == dt and np.array_equal(a, w)
    with pytest.raises(ValueError):
        t.link_trace_round(tie["ht"], tie["pb"], None, [tie["n_links"]])
    # more records than the first call's guess: the second call at the reported total
    gp = LC.path_graph(64)
    tp = _net(gp, ctx).compute_shortest_path_tree([0])
    hp = synth.make_hosts(64, 64)
    ppk = dict(src=np.zeros(40, np.uint32), dst_ip=np.full(40, hp["ip"][63], np.uint32),
               send_time=np.arange(40, 0, -1).astype(np.uint64))
    got = tp.link_trace_round(_host_table(hp, ctx), _batch(ppk))
    assert int(got[0][-1]) == 40 * 63 > 8 * 40 + 64
    want = XR.trace(gp, tp.nodes, (0, 1), tp.pred, tp.latency_ns, hp, ppk)
    for a, w in zip(got, want):
        assert np.array_equal(a, w)
