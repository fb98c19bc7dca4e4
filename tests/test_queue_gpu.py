"""Link queues on the card (sg_link_queue, shadow_amd.link_queue, PathTree.link_queue_round,
Group.link_queue_round) against tests/queue_ref.py.

Every output starts from sentinel values and is compared with np.array_equal; unless a test says
otherwise each case runs in host and in device mode and in both kernel forms (the flat segmented
scan and, under SG_LINK_QUEUE_SERIAL = 1, the lane per link).  Inputs are hand-made trace arrays
(tests/queue_cases.py) except in the last section; test_queue_ref_cpu.py qualifies them."""
import numpy as np
import pytest

import group_trace_cases as GC
import link_cases as LC
import queue_cases as QC
import queue_ref as QR
import sweep_cases as WC
import trace_cases as XC
import trace_ref as XR
from queue_gpu_calls import (FORMS, INPUTS, PY_FIELDS, VIEW, _batch, _call, _check_calls, _form, _host_table, _net, _pair,
                             _sentinels, _untouched, ctx_error)

pytestmark = pytest.mark.gpu

MAX = QR.MAX


def _check(ctx, monkeypatch, c, want=None, *, devs=(True, False), forms=FORMS, names=QR.FIELDS):
    """The case in every mode and form against the reference (the loop unless `want` is given)."""
    if want is None:
        rc, _, want = QC.ref(c)
        assert rc == QR.OK
    _check_calls(ctx, monkeypatch, c, {k: getattr(want, k) for k in names}, names, devs=devs, forms=forms)
    return want


# ---- 1. segment lengths
@pytest.mark.parametrize("n", QC.LENGTHS)
def test_one_segment(ctx, monkeypatch, n):
    """One link of n records: under, at and over a wave, a workgroup's lanes and a tile; three
    tiles and a record.  free_in inside the arrivals."""
    c = QC.random_trace([n], 100 + n, free_max=200, costs=(500,))
    want = _check(ctx, monkeypatch, c)
    assert n < 64 or (want.wait.any() and (want.wait == 0).any())


def test_packed_segments(ctx, monkeypatch):
    """The same lengths back to back, an empty link between every two, an empty first and an empty
    last link: the empty links keep their free_in value and zero sums."""
    c = QC.random_trace(QC.packed_lengths(), 5, free_max=100)
    want = _check(ctx, monkeypatch, c)
    empty = np.diff(c["link_off"].astype(np.int64)) == 0
    assert empty[0] and empty[-1] and np.array_equal(want.link_free[empty], c["free_in"][empty])
    assert want.ahead.max() >= 64 and not want.busy[empty].any()
    _check(ctx, monkeypatch, dict(c, free_in=None), devs=(True,))


# ---- 2. tile edges
def test_tile_edges(ctx, monkeypatch):
    """A segment ending exactly at a tile edge with the next starting there; a one-record segment
    on either side of the next edge; and all of it shifted by a leading segment of 1 .. 9 records,
    which moves the lanes' own eight-record edges across the segments'."""
    lengths = QC.tile_edge_lengths()
    assert sum(lengths[:2]) == QC.TILE and sum(lengths[:4]) == 2 * QC.TILE
    _check(ctx, monkeypatch, QC.random_trace(lengths, 6, free_max=100))
    for lead in range(1, 10):
        _check(ctx, monkeypatch, QC.random_trace([lead] + lengths, 6 + lead, free_max=100), devs=(True,), forms=("scan",))


# ---- 3. the carry past 1,024 tile aggregates
@pytest.mark.parametrize("shape", ["one", "mid", "three"])
def test_second_trip(ctx, monkeypatch, shape):
    """2,097,153 records, one more tile than the carry kernel's 1,024 threads take at once: one
    segment, 1,025 segments of 2,046, segments of 3.  Device mode, the closed form as the
    reference.  The lane-per-link form runs where a lane's segment is short (one lane looping
    over two million records takes seconds)."""
    c = QC.second_trip(shape)
    assert len(c["enter"]) == QC.SECOND_TRIP == 2_097_153
    want = QC.ref(c, closed=True)
    assert want.wait.any() and (want.wait == 0).any() and want.ahead.max() > 1
    _check(ctx, monkeypatch, c, want, devs=(True,), forms=("scan",) if shape == "one" else FORMS)


# ---- 4. arithmetic
def test_cost_zero(ctx, monkeypatch):
    """A link that serves in no time: nothing waits unless free_in says so, done is the start."""
    c = QC.random_trace([300, 0, 700], 7, costs=(0,), free_max=500)
    want = _check(ctx, monkeypatch, c)
    assert not want.busy.any() and np.array_equal(want.done, np.maximum(c["enter"], np.repeat(c["free_in"][[0, 2]], [300, 700])))


def test_ceiling(ctx, monkeypatch):
    """Costs 1, 80, 999, 1,000 and 1,001 ps with weights 0, 1, 1,500 and 2^32 - 1: every pair
    twice on a link of its cost, arrivals 1 ns apart (the second of a pair waits for the first)."""
    costs = (1, 80, 999, 1000, 1001)
    weight = np.uint32([0, 1, 1500, 2**32 - 1])
    packet = np.tile(np.repeat(np.arange(4), 2), len(costs))
    enter = np.tile(10 + np.arange(8), len(costs))
    c = QC.case(np.arange(len(costs) + 1) * 8, enter, packet, weight, costs)
    want = _check(ctx, monkeypatch, c)
    s = [[QR.service(w, k) for w in weight.tolist()] for k in costs]
    assert s[0] == [0, 1, 2, 4294968] and s[2][1:3] == [1, 1499] and s[4][1:] == [2, 1502, 4299262263]
    assert want.busy.tolist() == [2 * sum(r) for r in s]


def test_wide_products(ctx, monkeypatch):
    """w * cost past 2^64 with the quotient still below it (the 96-bit division), a record per
    link; times on both sides of 2^32 and of 2^63."""
    weight = np.uint32([2**32 - 1, 1000, 999, 5])
    costs = np.uint64([2**40, 2**62, 2**62 + 7, 2**62 + 12345])
    assert all(int(w) * int(k) >= 2**64 and QR.service(w, k) < MAX // 2 for w, k in zip(weight, costs))
    _check(ctx, monkeypatch, QC.case(np.arange(5), [5, 2**32, 2**33, 7], np.arange(4), weight, costs))
    for base in (2**32, 2**63):
        c = QC.random_trace([500, 400], 8, t0=base - 3000, free_max=6000)
        want = _check(ctx, monkeypatch, c)
        assert int(c["enter"].min()) < base < int(c["enter"].max()) and int(want.done.max()) > base and want.wait.any()


def test_free_in(ctx, monkeypatch):
    """link_free_in below, inside and above a segment's arrival times, and NULL."""
    c = QC.random_trace([400] * 4, 9)
    lo, hi = int(c["enter"].min()), int(c["enter"].max())
    free = np.uint64([0, lo - 1, (lo + hi) // 2, hi + 1000])
    want = _check(ctx, monkeypatch, dict(c, free_in=free))
    none = _check(ctx, monkeypatch, dict(c, free_in=None))
    first = c["link_off"][:-1].astype(np.int64)
    assert np.array_equal(want.wait[first[:2]], none.wait[first[:2]]) and (want.wait[first[2:]] > none.wait[first[2:]]).all()
    assert (want.wait[first[3]:] > hi - c["enter"][first[3]:].astype(np.int64)).all()


# ---- 5. chaining
def test_chaining(ctx, monkeypatch):
    """out_link_free fed back as link_free_in on every segment split in two equals one call on
    the whole segments (wait, done, the final free time; busy adds up)."""
    c = QC.random_trace([901, 0, 4100, 1], 10, free_max=300)
    whole = _check(ctx, monkeypatch, c)
    off = c["link_off"].astype(np.int64)
    cut = off[:-1] + np.diff(off) // 2
    a_idx = np.concatenate([np.arange(off[k], cut[k]) for k in range(4)])
    b_idx = np.concatenate([np.arange(cut[k], off[k + 1]) for k in range(4)])
    for form in FORMS:
        _form(monkeypatch, form)
        parts, free = [], c["free_in"]
        for idx, lens in ((a_idx, cut - off[:-1]), (b_idx, off[1:] - cut)):
            part = dict(c, link_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), enter=c["enter"][idx],
                        packet=c["packet"][idx], free_in=free)
            rc, outs = _call(ctx, part, dev=True)
            assert rc == 0
            parts.append(outs)
            free = outs["link_free"]
        for k in ("wait", "done"):
            got = np.empty_like(getattr(whole, k))
            got[a_idx], got[b_idx] = parts[0][k], parts[1][k]
            assert np.array_equal(got, getattr(whole, k)), k
        assert np.array_equal(parts[1]["link_free"], whole.link_free)
        assert np.array_equal(parts[0]["busy"] + parts[1]["busy"], whole.busy)


# ---- 6. queue shapes
def test_queue_shapes(ctx, monkeypatch):
    """Every record at one time: the wait is the prefix of the services, ahead_i = i.  A link idle
    between all its records: no wait, nobody ahead.  Bursts separated by idle gaps."""
    n = 3000
    rng = np.random.default_rng(11)
    weight = rng.integers(1, 50, n).astype(np.uint32)
    c = QC.case([0, n], np.full(n, 777), np.arange(n), weight, [1000])
    want = _check(ctx, monkeypatch, c)
    assert np.array_equal(want.ahead, np.arange(n)) and np.array_equal(want.wait, np.cumsum(weight) - weight)
    idle = QC.case([0, n], 777 + 50 * np.arange(n), np.arange(n), weight, [1000])
    want = _check(ctx, monkeypatch, idle)
    assert not want.wait.any() and not want.ahead.any() and int(want.busy[0]) == int(weight.sum())
    # bursts of 100 records 1 ns apart, 10 us between bursts (a burst takes about 2.5 us to serve)
    burst = QC.case([0, n], 777 + (np.arange(n) // 100) * 10_000 + np.arange(n) % 100, np.arange(n), weight, [1000])
    want = _check(ctx, monkeypatch, burst)
    assert not want.wait[::100].any() and want.wait[99::100].all() and int(want.ahead_max[0]) > 90
    assert (want.ahead[::100] == 0).all()


# ---- 7. unsorted input
def test_unsorted(ctx, monkeypatch):
    """The recurrence takes the records as given: shuffled arrival times give the loop's result
    (done still never falls, so ahead is what the definition counts)."""
    c = QC.random_trace([0, 2500, 70, 1, 3000], 12, free_max=100)
    rng = np.random.default_rng(13)
    enter = c["enter"].copy()
    off = c["link_off"].astype(np.int64)
    for k in range(len(off) - 1):
        rng.shuffle(enter[off[k]:off[k + 1]])
    assert (np.diff(enter[off[1]:off[2]].astype(np.int64)) < 0).any()
    _check(ctx, monkeypatch, dict(c, enter=enter))


# ---- 8. subsets and sizes
def test_output_subsets(ctx, monkeypatch):
    """Each output alone, all together, the pairs that share work (ahead without done, the maximum
    of ahead alone); unit weights with and without a packet array; no record at all."""
    from shadow_amd import _capi

    c = QC.random_trace([0, 700, 3, 0, 2600, 0], 14, free_max=100)
    for names in [(k,) for k in QR.FIELDS] + [("ahead", "ahead_max"), ("wait", "busy"), QR.FIELDS]:
        _check(ctx, monkeypatch, c, names=names, devs=(True,))
    _check(ctx, monkeypatch, c, names=("ahead", "link_free"), devs=(False,))
    unit = dict(c, weight=None)
    want = _check(ctx, monkeypatch, unit)
    assert np.array_equal(_check(ctx, monkeypatch, dict(unit, packet=None)).done, want.done)
    empty = QC.case([0, 0, 0, 0], [], None, None, [5, 6, 7], [9, 8, 7])
    want = _check(ctx, monkeypatch, empty)
    assert want.link_free.tolist() == [9, 8, 7] and not want.busy.any()
    for dev in (True, False):
        rc, outs = _call(ctx, dict(empty, free_in=None), ("link_free", "ahead_max"), dev=dev)
        assert rc == _capi.SG_OK and not outs["link_free"].any() and not outs["ahead_max"].any()


# ---- 9. errors
@pytest.mark.parametrize("dev", [True, False], ids=["device", "host"])
def test_argument_errors(ctx, monkeypatch, dev):
    """SG_ERR_INVALID_ARG with every output untouched: NULL ctx, link_off, enter_ns or cost_ps; no
    output; weight without packet; out_link_free == link_free_in."""
    from shadow_amd import _capi

    c, _ = QC.hand()
    assert _call(ctx, c, dev=dev)[0] == _capi.SG_OK
    rc, outs = _call(ctx, c, dev=dev, handle=False)
    assert rc == _capi.SG_ERR_INVALID_ARG and _untouched(outs)
    rc, outs = _call(ctx, dict(c, packet=None), dev=dev)
    assert rc == _capi.SG_ERR_INVALID_ARG and _untouched(outs) and "weight without packet" in ctx_error(ctx)
    rc, outs = _call(ctx, c, (), dev=dev)
    assert rc == _capi.SG_ERR_INVALID_ARG and "no output" in ctx_error(ctx)
    rc, outs = _call(ctx, c, ("wait", "busy"), dev=dev, alias_free=True)
    assert rc == _capi.SG_ERR_INVALID_ARG and _untouched(outs)
    for name in ("link_off", "enter", "cost_ps"):
        rc, outs = _call_without(ctx, c, name, dev)
        assert rc == _capi.SG_ERR_INVALID_ARG and _untouched(outs), name


def _call_without(ctx, c, name, dev):
    """_call with one required input NULL (the sizes taken from the full case)."""
    import torch

    from shadow_amd import _capi

    C = _capi.C
    outs = _sentinels(c, QR.FIELDS)
    keep = []

    def ptr(a):
        if not dev:
            return C.c_void_p(a.ctypes.data)
        keep.append(torch.from_numpy(a.view(VIEW[a.dtype]).copy()).cuda())
        return C.c_void_p(keep[-1].data_ptr())

    ip = [None if k == name else ptr(c[k]) for k in INPUTS]
    op = [ptr(outs[k]) for k in QR.FIELDS]
    if dev:
        torch.cuda.synchronize()
    rc = _capi.load().sg_link_queue(ctx.handle, _capi.SG_ROUTE_OUT_DEVICE if dev else 0, len(c["link_off"]) - 1, ip[0],
                                    len(c["enter"]), ip[1], ip[2], ip[3], len(c["weight"]), ip[4], ip[5], *op)
    if dev:
        torch.cuda.synchronize()
        for k, t in zip(QR.FIELDS, keep[-len(op):]):
            outs[k][...] = t.cpu().numpy().view(outs[k].dtype)
    return rc, outs


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dev", [True, False], ids=["device", "host"])
def test_data_errors(ctx, monkeypatch, dev, form):
    """A bad link_off with its link (host mode: every output untouched; device mode: found by the
    first kernel, the smallest link, and nothing is indexed by it, however wild the value); a
    packet index past the weights, the smallest; done reaching 2^64 - 1, the smallest; and the
    precedence link_off, packet, overflow.  Codes and pairs are the reference's."""
    _form(monkeypatch, form)
    c, _ = QC.hand()
    pk = c["packet"].copy()
    pk[[3, 5]] = 3, 9
    free = c["free_in"].copy()
    free[0] = MAX - 20
    late = free.copy()
    late[0] = MAX - 21
    wild = np.uint64([0, 2**40, 4, 6])
    cases = [dict(c, link_off=np.uint64(off)) for off in ([1, 4, 4, 6], [0, 4, 3, 6], [0, 4, 4, 5], [0, 4, 4, 7], [0, 5, 4, 7])]
    cases += [dict(c, link_off=wild), dict(c, link_off=wild, packet=pk, free_in=free), dict(c, packet=pk),
              dict(c, packet=pk, free_in=free), dict(c, free_in=free), dict(c, free_in=late),
              dict(c, cost_ps=np.uint64([2**64 - 1, 1, 1]), weight=np.uint32([3, 1, 1000]))]
    seen = set()
    for bad in cases:
        code, pair, _ = QC.ref(bad)
        assert code != QR.OK
        rc, outs = _call(ctx, bad, dev=dev)
        assert (rc, _pair(ctx)) == (code, pair), (bad["link_off"], ctx_error(ctx))
        if not dev and pair[1] == QR.UMAX:
            assert _untouched(outs)
        seen.add((code, pair[1] == QR.UMAX))
    assert len(seen) == 3
    # the call after an error is a good one
    rc, outs = _call(ctx, c, dev=dev)
    assert rc == 0 and np.array_equal(outs["done"], QC.hand()[1].done)
    # done = 2^64 - 2 is no error
    ok = dict(c, free_in=np.uint64([MAX - 28, 77, 100]))
    code, _, want = QC.ref(ok)
    assert code == QR.OK and int(want.done[3]) == MAX - 1
    rc, outs = _call(ctx, ok, dev=dev)
    assert rc == 0 and all(np.array_equal(outs[k], getattr(want, k)) for k in QR.FIELDS)


# ---- 10. real traces
def _same_result(got, want):
    """A LinkQueueResult against the reference's Result, or against another LinkQueueResult."""
    for a, b in PY_FIELDS.items():
        x, w = getattr(got, a), getattr(want, b if hasattr(want, b) else a)
        assert x.dtype == w.dtype and np.array_equal(x, w), a


@pytest.mark.parametrize("which", ["tie", "wide"])
def test_path_tree_round(ctx, oracle, monkeypatch, which):
    """trace_cases.tie_round() and wide_round() through PathTree.link_queue_round, payload
    weights: the trace is trace_ref's, the queue queue_ref's over it; both forms; a watch list."""
    g = XC.wide_graph() if which == "wide" else LC.tie_graph()
    hosts, pk = XC.wide_round() if which == "wide" else XC.tie_round()[:2]
    net = _net(g, ctx)
    t = net.compute_shortest_path_tree()
    nl = XR.n_links(g)
    cost = QC.WIDE_COST if which == "wide" else QC.TIE_COST
    ht, pb = _host_table(hosts, ctx), _batch(pk)
    tr = XR.trace(g, t.nodes, (0, g["n"]), t.pred, t.latency_ns, hosts, pk)
    rc, _, want = QR.loop(tr[0], tr[3], tr[1], pk["payload"], cost_ps=np.full(nl, cost, np.uint64))
    assert rc == QR.OK and all(QC.conditions(tr[0], want))
    for form in FORMS:
        _form(monkeypatch, form)
        got = t.link_queue_round(ht, pb, None, "payload", cost_ps=cost)
        assert all(np.array_equal(a, b) for a, b in zip(got[:5], tr))
        _same_result(got[5], want)
    # unit weights, a free time per link and a watch list: the other links own nothing
    some = [5, 17, nl - 1] + np.argsort(np.diff(tr[0].astype(np.int64)))[-3:].tolist()
    free = np.random.default_rng(3).integers(0, int(tr[3].max()), nl).astype(np.uint64)
    tw = XR.trace(g, t.nodes, (0, g["n"]), t.pred, t.latency_ns, hosts, pk, watch=some)
    costs = np.full(nl, cost * 700, np.uint64)
    rc, _, want = QR.loop(tw[0], tw[3], cost_ps=costs, free_in=free)
    assert rc == QR.OK and want.wait.any()
    got = t.link_queue_round(ht, pb, cost_ps=costs, watch=some, free_ns=free)
    assert all(np.array_equal(a, b) for a, b in zip(got[:5], tw))
    _same_result(got[5], want)


@pytest.mark.parametrize("name", WC.NAMES)
def test_sweep(ctx, oracle, monkeypatch, name):
    """The 40 generated graphs, queue_cases.sweep_round from row 0's hosts, one cost per link
    drawn from {0, 80, 8,000, 10^6} ps, payload weights: sg_link_trace_packets on host arrays,
    then shadow_amd.link_queue on its output; both forms."""
    import shadow_amd
    from shadow_amd import _capi

    C = _capi.C
    c, r = WC.case(name), WC.refs(oracle, name)[0]
    g, n = c["g"], c["g"]["n"]
    pk, status = QC.sweep_round(c)
    nl = XR.n_links(g)
    cost = QC.sweep_costs(name, nl)
    tr = XR.trace(g, c["nodes"], (0, n), r["pred"], r["lat"], c["hosts"], pk, status)
    rc, _, want = QR.loop(tr[0], tr[3], tr[1], pk["payload"], cost_ps=cost)
    assert rc == QR.OK
    net, ht, pb = _net(g, ctx), _host_table(c["hosts"], ctx), _batch(pk)
    import torch

    d_status = torch.from_numpy(status).cuda()
    torch.cuda.synchronize()
    cap = len(tr[1])
    off, pkt, enter = np.zeros(nl + 1, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.uint64)
    total = C.c_uint64()
    p = pb.c_struct()
    pred, lat = np.ascontiguousarray(r["pred"], np.uint32), np.ascontiguousarray(r["lat"], np.uint64)
    _capi.check(ctx.handle, _capi.load().sg_link_trace_packets(
        ctx.handle, net._ensure_net(), ht.handle, c["nodes"].ctypes.data, n, 0, n, 0, pred.ctypes.data, lat.ctypes.data,
        C.byref(p), C.c_void_p(d_status.data_ptr()), None, off.ctypes.data, pkt.ctypes.data, None, enter.ctypes.data, None,
        cap, C.byref(total)))
    assert total.value == cap and np.array_equal(off, tr[0]) and np.array_equal(pkt, tr[1]) and np.array_equal(enter, tr[3])
    for form in FORMS:
        _form(monkeypatch, form)
        _same_result(shadow_amd.link_queue(ctx, off, enter, pkt, pk["payload"], cost_ps=cost), want)


@pytest.fixture(scope="module")
def tie_single(ctx):
    """The tie round with queue_cases.group_status through PathTree.link_queue_round: what the
    group's result must equal bit for bit."""
    g = LC.tie_graph()
    hosts, pk, mixed = XC.tie_round()
    net = _net(g, ctx)
    t = net.compute_shortest_path_tree()
    return dict(g=g, hosts=hosts, pk=pk, status=QC.group_status(mixed), net=net, tree=t)


@pytest.mark.parametrize("world", QC.GROUP_WORLDS)
def test_group_round(ctx, tie_single, world):
    """Group.link_queue_round over 1 and 3 members on one device: the reference on the members'
    batches concatenated, and the single call on that batch bit for bit."""
    from test_group_trace_gpu import members

    s = tie_single
    g, hosts, t = s["g"], s["hosts"], s["tree"]
    nl = XR.n_links(g)
    parts = GC.split(hosts, s["pk"], s["status"], g["n"], world)
    cat, cstatus, _ = GC.concat(parts)
    single = t.link_queue_round(_host_table(hosts, ctx), _batch(cat), cstatus, "payload", cost_ps=QC.TIE_COST)
    tr = XR.trace(g, t.nodes, (0, g["n"]), t.pred, t.latency_ns, hosts, cat, cstatus)
    rc, _, want = QR.loop(tr[0], tr[3], tr[1], cat["payload"], cost_ps=np.full(nl, QC.TIE_COST, np.uint64))
    assert rc == QR.OK and all(QC.conditions(tr[0], want))
    _same_result(single[5], want)
    with members(world) as (ctxs, group, keep):
        graphs = [keep(_net(g, c)) for c in ctxs]
        hts = [keep(_host_table(hosts, c)) for c in ctxs]
        batches = [_batch(p[0]) for p in parts]
        got = group.link_queue_round(graphs, hts, t, batches, [p[1] for p in parts], "payload", cost_ps=QC.TIE_COST,
                                     root=world - 1)
        assert len(got) == 7
        for k, j in ((0, 0), (1, 1), (3, 2), (4, 3), (5, 4)):  # (the group's tuple has the member after the packet)
            assert np.array_equal(got[k], single[j]) and np.array_equal(got[k], tr[j])
        assert np.array_equal(got[2], GC.members_of(got[1], GC.concat(parts)[2]))
        _same_result(got[6], single[5])
        _same_result(got[6], want)
        # per-member arrays for the weights, one of them left to 1 per packet
        ws = [p[0]["payload"] if m != 0 else None for m, p in enumerate(parts)]
        cw = np.concatenate([p[0]["payload"] if m != 0 else np.ones(len(p[0]["payload"]), np.uint32) for m, p in enumerate(parts)])
        rc, _, want = QR.loop(tr[0], tr[3], tr[1], cw, cost_ps=np.full(nl, QC.TIE_COST, np.uint64))
        _same_result(group.link_queue_round(graphs, hts, t, batches, [p[1] for p in parts], ws, cost_ps=QC.TIE_COST)[6], want)
