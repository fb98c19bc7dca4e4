"""Carried link queues on the card (sg_link_queue with its carry flag, and carry=True of
shadow_amd.link_queue, PathTree.link_queue_round and Group.link_queue_round) against
tests/queue_carry_ref.py.

Every output starts from sentinel values and is compared with np.array_equal; unless a test says
otherwise each case runs in host and in device mode and in both forms of the scan (the flat
segmented scan and, under SG_LINK_QUEUE_SERIAL = 1, the lane per link).  The reference is the
event-driven simulation; the fixed-point loop gives the iteration counts.  Inputs:
tests/queue_carry_cases.py; test_queue_carry_ref_cpu.py qualifies them."""
import functools

import numpy as np
import pytest

import group_trace_cases as GC
import link_cases as LC
import queue_carry_cases as CC
import queue_carry_ref as CR
import queue_cases as QC
import queue_gpu_calls as QG
import queue_ref as QR
import sweep_cases as WC
import trace_cases as XC
import trace_ref as XR
from queue_gpu_calls import (CARRY, FORMS, INPUTS, PY_FIELDS, VIEW, _batch, _check_calls, _form, _host_table, _net, _pair,
                             _sentinels, _untouched, ctx_error)

pytestmark = pytest.mark.gpu

MAX = QR.MAX
_call = functools.partial(QG._call, carry=True)


def _check(ctx, monkeypatch, c, want=None, *, devs=(True, False), forms=FORMS, names=QR.FIELDS, iters=None):
    """The case in every mode and form against the reference (the event simulation unless `want`
    is given); iters: the iterations every call must have taken."""
    if want is None:
        rc, _, want, _, _ = CC.ref(c)
        assert rc == CR.OK
    _check_calls(ctx, monkeypatch, c, {k: getattr(want, k) for k in names}, names, carry=True, devs=devs, forms=forms,
                 iters=iters)
    return want


# ---- 1. the definition's own examples
def test_hand_example(ctx, monkeypatch):
    """Packet A waits behind B on link 0 and reaches link 1 after C.  Fails where the flag is
    ignored: the first-order result serves A ahead of C."""
    c, want, _, first = CC.hand()
    _check(ctx, monkeypatch, c, want, iters=2)
    assert not np.array_equal(want.done, first.done)
    rc, outs = _call(ctx, c, dev=True, carry=False)
    assert rc == 0 and all(np.array_equal(outs[k], getattr(first, k)) for k in QR.FIELDS)


def test_cost_zero(ctx, monkeypatch):
    """Every cost 0, no link_free_in: the input comes back, all waits 0, one iteration."""
    c = CC.random_chains(5, n_links=5, n_packets=80, costs=(0,))
    want = _check(ctx, monkeypatch, c, iters=1)
    assert not want.wait.any() and np.array_equal(want.done, c["enter"])


def test_single_record_chains(ctx, monkeypatch):
    """A packet per record, sorted segments: the unflagged call's result, bit for bit."""
    c = CC.single_records([0, 70, 300, 1, 2100], 31)
    want = _check(ctx, monkeypatch, c, iters=1)
    for dev in (True, False):
        rc, outs = _call(ctx, c, dev=dev, carry=False)
        assert rc == 0 and all(np.array_equal(outs[k], getattr(want, k)) for k in QR.FIELDS)


@pytest.mark.parametrize("k", CC.STAIRS)
def test_staircase(ctx, monkeypatch, k):
    """k packets, each late on its second link only once the one before is known to be: the
    library takes the reference loop's iterations, at least k."""
    c = CC.staircase(k)
    rc, _, want, _, iters = CC.ref(c, jacobi=True)
    assert rc == CR.OK and iters >= k
    _check(ctx, monkeypatch, c, want, iters=iters)


# ---- 2. sort tiers and tile edges
def test_segment_lengths(ctx, monkeypatch):
    """Link segments of 0, 1, 64, 65, 2,047, 2,048, 2,049 and 3 x 2,048 + 1 records, fed by chains
    of 1 to 3 records: the wave sort, the LDS sort up to a full piece, the merge of two and of four
    pieces, and the scan's tile edges, on an order that changes between iterations."""
    c = CC.from_lengths(CC.SEGMENTS, 4, free_max=500)
    want = _check(ctx, monkeypatch, c)
    assert want.wait.any() and (want.wait == 0).any()


def test_long_chains(ctx, monkeypatch):
    """One packet with a chain of 2,049 records and one with 65: the packet sort's merge and LDS
    tiers (the others, of 1 to 3 records, take the wave tier)."""
    c = CC.long_chains()
    want = _check(ctx, monkeypatch, c, devs=(True,))
    assert want.wait.any()
    _check(ctx, monkeypatch, c, want, devs=(False,), forms=("scan",))


def test_hot_link(ctx, monkeypatch):
    """One link of 5,000 records behind 50 slow feeders: its order changes from one iteration to
    the next (three pieces merged anew every time)."""
    _check(ctx, monkeypatch, CC.hot_link())


# ---- 3. link_free_in, the order given, the outputs taken
def test_free_in(ctx, monkeypatch):
    """link_free_in below, inside and above a link's arrivals, and NULL."""
    c = CC.random_chains(9, n_links=4, n_packets=300, hops=(1, 3), span=3000)
    lo, hi = int(c["enter"].min()), int(c["enter"].max())
    free = np.uint64([0, max(lo, 1) - 1, (lo + hi) // 2, hi + 1000])
    want = _check(ctx, monkeypatch, dict(c, free_in=free))
    none = _check(ctx, monkeypatch, dict(c, free_in=None))
    off = c["link_off"].astype(np.int64)
    assert off[4] > off[3] and int(want.wait_max[3]) >= 1000 and int(want.wait_sum[2]) > int(none.wait_sum[2])

def test_shuffled_input(ctx, monkeypatch):
    """Every link's records in a random order: the outputs follow their records."""
    c = CC.random_chains(7, n_links=6, n_packets=900, hops=(1, 4), span=5000)
    want = _check(ctx, monkeypatch, c, devs=(True,))
    s, perm = CC.shuffled(c, 8)
    got = _check(ctx, monkeypatch, s)
    for k in QR.RECORD_FIELDS:
        assert np.array_equal(getattr(got, k), getattr(want, k)[perm]), k
    assert np.array_equal(got.link_free, want.link_free)


def test_output_subsets(ctx, monkeypatch):
    """Each output alone, the pairs that share work, all together; unit weights; no record."""
    from shadow_amd import _capi

    c = CC.random_chains(14, n_links=7, n_packets=600, hops=(1, 4), span=4000, free_max=200)
    for names in [(k,) for k in QR.FIELDS] + [("ahead", "ahead_max"), ("wait", "busy")]:
        _check(ctx, monkeypatch, c, names=names, devs=(True,), forms=("scan",))
    _check(ctx, monkeypatch, c, names=("ahead", "link_free"), devs=(False,))
    _check(ctx, monkeypatch, dict(c, weight=None))
    empty = dict(QC.case([0, 0, 0, 0], [], [], None, [5, 6, 7], [9, 8, 7]), n_packets=0)
    for dev in (True, False):
        rc, outs = _call(ctx, empty, dev=dev)
        assert rc == _capi.SG_OK and outs["link_free"].tolist() == [9, 8, 7] and not outs["busy"].any()
        assert not outs["ahead_max"].any() and not outs["wait_max"].any()


# ---- 4. errors
@pytest.mark.parametrize("dev", [True, False], ids=["device", "host"])
def test_argument_errors(ctx, dev):
    """With the flag, every output untouched: NULL packet (SG_ERR_INVALID_ARG), a record count past
    2^32 - 2 (SG_ERR_CAPACITY, refused before any array is read), today's argument errors, a
    host-mode bad link_off."""
    from shadow_amd import _capi

    c, _, _, _ = CC.hand()
    rc, outs = _call(ctx, dict(c, packet=None, weight=None), dev=dev)
    assert rc == _capi.SG_ERR_INVALID_ARG and _untouched(outs) and "without packet" in ctx_error(ctx)
    rc, outs = _call(ctx, dict(c, packet=None), dev=dev)
    assert rc == _capi.SG_ERR_INVALID_ARG and _untouched(outs)
    rc, outs = _call(ctx, c, (), dev=dev)
    assert rc == _capi.SG_ERR_INVALID_ARG and "no output" in ctx_error(ctx)
    rc, outs = _call(ctx, c, dev=dev, n_records=2**32 - 1)
    assert rc == _capi.SG_ERR_CAPACITY and _untouched(outs)
    if not dev:
        rc, outs = _call(ctx, dict(c, link_off=np.uint64([0, 3, 2, 6])), dev=dev)
        assert (rc, _pair(ctx)) == (_capi.SG_ERR_INVALID_ARG, (1, QR.UMAX)) and _untouched(outs)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dev", [True, False], ids=["device", "host"])
def test_data_errors(ctx, monkeypatch, dev, form):
    """A bad link_off; a packet index not below n_weights, with and without weights; two records
    of one packet at one time; done, and done + gap alone, reaching 2^64 - 1; and the precedence
    link_off, packet, twin, overflow.  Codes and pairs are the reference's."""
    _form(monkeypatch, form)
    c, want, _, _ = CC.hand()
    pk = c["packet"].copy()
    pk[[3, 4]] = 3, 7
    twin = np.uint64([100, 101, 106, 100, 100, 107])
    twins = np.uint64([100, 100, 100, 100, 100, 100])  # (every record has one: the smallest is record 0)
    far = np.uint64([0, MAX - 12, 0])
    wild = np.uint64([0, 2**40, 4, 6])
    cases = [dict(c, link_off=wild), dict(c, link_off=wild, packet=pk, enter=twin, free_in=far),
             dict(c, link_off=np.uint64([0, 2, 4, 5]), packet=pk),
             dict(c, packet=pk), dict(c, packet=pk, enter=twin, free_in=far), dict(c, packet=pk, weight=None, n_packets=7),
             dict(c, enter=twin), dict(c, enter=twin, free_in=far), dict(c, enter=twins), dict(c, free_in=far),
             CC.carry_overflow(0)]
    if dev is False:
        cases = cases[3:]  # (a bad host link_off is an argument error: test_argument_errors)
    seen = set()
    for bad in cases:
        code, pair, _, _, _ = CC.ref(bad)
        assert code != CR.OK
        rc, outs = _call(ctx, bad, dev=dev)
        assert rc == code, (bad, ctx_error(ctx))
        assert pair is None or _pair(ctx) == pair, (bad, ctx_error(ctx))
        seen.add((code, pair is None, pair is not None and pair[1] == QR.UMAX))
    assert len(seen) == (3 if dev else 2)
    # the call after an error is a good one; and the 2^64 - 2 that is no error
    rc, outs = _call(ctx, c, dev=dev)
    assert rc == 0 and all(np.array_equal(outs[k], getattr(want, k)) for k in QR.FIELDS)
    ok = CC.carry_overflow(1)
    rc, outs = _call(ctx, ok, dev=dev)
    assert rc == 0 and outs["done"].tolist() == [MAX - 6, MAX - 1]
    ok = dict(c, packet=pk, weight=None, n_packets=8)
    rc, outs = _call(ctx, ok, dev=dev)
    assert rc == 0 and all(np.array_equal(outs[k], getattr(CC.ref(ok)[2], k)) for k in QR.FIELDS)


def test_iteration_cap(ctx, monkeypatch):
    """SG_LINK_QUEUE_CARRY_ITERS = 2 on the 6-staircase: SG_ERR_CAPACITY with the pair (2,
    UINT32_MAX), never a partial answer; unset, the same case converges."""
    from shadow_amd import _capi

    c = CC.staircase(6)
    monkeypatch.setenv("SG_LINK_QUEUE_CARRY_ITERS", "2")
    for dev in (True, False):
        rc, outs = _call(ctx, c, dev=dev)
        assert (rc, _pair(ctx)) == (_capi.SG_ERR_CAPACITY, (2, QR.UMAX)) and "SG_LINK_QUEUE_CARRY_ITERS" in ctx_error(ctx)
        assert dev or _untouched(outs)
    assert CC.ref(c, jacobi=True, cap=2)[:2] == (CR.CAPACITY, (2, QR.UMAX))
    monkeypatch.delenv("SG_LINK_QUEUE_CARRY_ITERS")
    _check(ctx, monkeypatch, c, forms=("scan",))


# ---- 5. a non-blocking stream
def test_non_blocking_stream():
    """The carried call on a context whose stream is the caller's non-blocking stream S
    (sg_ctx_set_stream, through Context(stream=)): the inputs reach the device on S behind a 30 ms
    delay (stream_cases.DELAY_CYCLES), so a launch or a copy on any other stream would read them
    before they are there; the outputs are read back on S."""
    import torch

    import stream_cases as SC
    from shadow_amd import Context, _capi

    C = _capi.C
    c = CC.random_chains(41, n_links=6, n_packets=700, hops=(1, 4), span=4000)
    rc, _, want, _, _ = CC.ref(c)
    assert rc == CR.OK and want.wait.any()
    S = torch.cuda.Stream()
    sctx = Context(0, stream=S.cuda_stream)
    try:
        outs = _sentinels(c, QR.FIELDS)
        pin = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(VIEW[a.dtype]).copy()).pin_memory()  # noqa: E731
        h_in = [None if c[k] is None else pin(c[k]) for k in INPUTS]
        h_out = {k: pin(outs[k]) for k in QR.FIELDS}
        with torch.cuda.stream(S):
            torch.cuda._sleep(SC.DELAY_CYCLES)
            d_in = [None if t is None else t.to("cuda", non_blocking=True) for t in h_in]
            d_out = {k: t.to("cuda", non_blocking=True) for k, t in h_out.items()}
            ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
            rc = _capi.load().sg_link_queue(sctx.handle, _capi.SG_ROUTE_OUT_DEVICE | CARRY, len(c["link_off"]) - 1, ptr(d_in[0]),
                                            len(c["enter"]), ptr(d_in[1]), ptr(d_in[2]), ptr(d_in[3]), c["n_packets"],
                                            ptr(d_in[4]), ptr(d_in[5]), *[ptr(d_out[k]) for k in QR.FIELDS])
            for k in QR.FIELDS:
                h_out[k].copy_(d_out[k], non_blocking=True)
            S.synchronize()
        _capi.check(sctx.handle, rc)
        for k in QR.FIELDS:
            assert np.array_equal(h_out[k].numpy().view(outs[k].dtype), getattr(want, k)), k
    finally:
        S.synchronize()
        sctx.close()


# ---- 6. real traces
def _same_carried(got, want, cur, iters=None):
    """A LinkQueueCarried against the reference's Result, carried enter and iterations."""
    for a, b in PY_FIELDS.items():
        x, w = getattr(got, a), getattr(want, b)
        assert x.dtype == w.dtype and np.array_equal(x, w), a
    assert got.enter_ns.dtype == np.uint64 and np.array_equal(got.enter_ns, cur)
    assert iters is None or got.iterations == iters


@pytest.fixture(scope="module")
def tie(ctx):
    """The tie round, its tree, its trace and the carried reference under queue_cases.TIE_COST."""
    g = LC.tie_graph()
    hosts, pk, mixed = XC.tie_round()
    net = _net(g, ctx)
    t = net.compute_shortest_path_tree()
    tr = XR.trace(g, t.nodes, (0, g["n"]), t.pred, t.latency_ns, hosts, pk)
    c = CC.case(tr[0], tr[3], tr[1], pk["payload"], np.full(XR.n_links(g), QC.TIE_COST, np.uint64))
    rc, _, want, cur, iters = CC.ref(c, jacobi=True)
    assert rc == CR.OK and all(CC.conditions(c, cur, iters))
    return dict(g=g, hosts=hosts, pk=pk, mixed=mixed, net=net, tree=t, tr=tr, case=c, want=want, cur=cur, iters=iters)


def test_path_tree_round(ctx, tie, monkeypatch):
    """The tie round through PathTree.link_queue_round(carry=True), payload weights, both forms:
    the trace is trace_ref's, the queue the carried reference's over it, the carried exit the
    trace's exit moved by done - enter.  Fails where the flag is ignored."""
    t, tr = tie["tree"], tie["tr"]
    ht, pb = _host_table(tie["hosts"], ctx), _batch(tie["pk"])
    for form in FORMS:
        _form(monkeypatch, form)
        got = t.link_queue_round(ht, pb, None, "payload", cost_ps=QC.TIE_COST, carry=True)
        assert len(got) == 7 and all(np.array_equal(a, b) for a, b in zip(got[:5], tr))
        _same_carried(got[5], tie["want"], tie["cur"], tie["iters"])
        assert np.array_equal(got[6], tr[4] + (tie["want"].done - tr[3]))
    # the raw call on the same trace, both modes; and the guard: without the flag the call gives
    # queue_ref.loop's first-order result as before
    _check(ctx, monkeypatch, tie["case"], tie["want"], forms=("scan",), iters=tie["iters"])
    rc, _, first = QC.ref(tie["case"])
    assert rc == QR.OK and not np.array_equal(first.done, tie["want"].done)
    got = t.link_queue_round(ht, pb, None, "payload", cost_ps=QC.TIE_COST)
    assert len(got) == 6
    for a, b in PY_FIELDS.items():
        assert np.array_equal(getattr(got[5], a), getattr(first, b)), a
    rc, outs = _call(ctx, tie["case"], dev=True, carry=False)
    assert rc == 0 and all(np.array_equal(outs[k], getattr(first, k)) for k in QR.FIELDS)


def test_path_tree_round_watch(ctx, tie):
    """A watch list, unit weights, a free time per link: an unwatched link is crossed at its
    latency (the gap between a packet's watched records spans it)."""
    g, t = tie["g"], tie["tree"]
    nl = XR.n_links(g)
    some = np.argsort(np.diff(tie["tr"][0].astype(np.int64)))[-12:].tolist()
    free = np.random.default_rng(3).integers(0, int(tie["tr"][3].max()), nl).astype(np.uint64)
    tw = XR.trace(g, t.nodes, (0, g["n"]), t.pred, t.latency_ns, tie["hosts"], tie["pk"], watch=some)
    c = CC.case(tw[0], tw[3], tw[1], None, np.full(nl, QC.TIE_COST * 700, np.uint64), free, n_packets=len(tie["pk"]["src"]))
    rc, _, want, cur, _ = CC.ref(c)
    assert rc == CR.OK and (cur != c["enter"]).any() and np.bincount(tw[1]).max() > 1
    got = t.link_queue_round(_host_table(tie["hosts"], ctx), _batch(tie["pk"]), cost_ps=c["cost_ps"], watch=some,
                             free_ns=free, carry=True)
    assert all(np.array_equal(a, b) for a, b in zip(got[:5], tw))
    _same_carried(got[5], want, cur)


@pytest.mark.parametrize("name", CC.SWEEP_NAMES)
def test_sweep(ctx, oracle, monkeypatch, name):
    """Six generated graphs, queue_cases.sweep_round, one cost per link drawn from {0, 80, 8,000,
    10^6} ps, payload weights: shadow_amd.link_queue(carry=True) on the reference trace."""
    import shadow_amd

    c, r = WC.case(name), WC.refs(oracle, name)[0]
    g, n = c["g"], c["g"]["n"]
    pk, status = QC.sweep_round(c)
    tr = XR.trace(g, c["nodes"], (0, n), r["pred"], r["lat"], c["hosts"], pk, status)
    k = CC.case(tr[0], tr[3], tr[1], pk["payload"], QC.sweep_costs(name, XR.n_links(g)))
    rc, _, want, cur, iters = CC.ref(k, jacobi=True)
    assert rc == CR.OK and all(CC.conditions(k, cur, iters))
    for form in FORMS:
        _form(monkeypatch, form)
        got = shadow_amd.link_queue(ctx, tr[0], tr[3], tr[1], pk["payload"], cost_ps=k["cost_ps"], carry=True)
        _same_carried(got, want, cur, iters)
    first = shadow_amd.link_queue(ctx, tr[0], tr[3], tr[1], pk["payload"], cost_ps=k["cost_ps"])
    assert not np.array_equal(first.done_ns, want.done)


@pytest.mark.parametrize("world", QC.GROUP_WORLDS)
def test_group_round(ctx, tie, world):
    """Group.link_queue_round(carry=True) over 1 and 3 members on one device: the reference on the
    members' batches concatenated, and the single call on that batch bit for bit."""
    from test_group_trace_gpu import members

    g, hosts, t = tie["g"], tie["hosts"], tie["tree"]
    status = QC.group_status(tie["mixed"])
    parts = GC.split(hosts, tie["pk"], status, g["n"], world)
    cat, cstatus, _ = GC.concat(parts)
    single = t.link_queue_round(_host_table(hosts, ctx), _batch(cat), cstatus, "payload", cost_ps=QC.TIE_COST, carry=True)
    tr = XR.trace(g, t.nodes, (0, g["n"]), t.pred, t.latency_ns, hosts, cat, cstatus)
    c = CC.case(tr[0], tr[3], tr[1], cat["payload"], np.full(XR.n_links(g), QC.TIE_COST, np.uint64))
    rc, _, want, cur, _ = CC.ref(c)
    assert rc == CR.OK and all(CC.conditions(c, cur, 3)[:2])
    _same_carried(single[5], want, cur)
    with members(world) as (ctxs, group, keep):
        graphs = [keep(_net(g, x)) for x in ctxs]
        hts = [keep(_host_table(hosts, x)) for x in ctxs]
        batches = [_batch(p[0]) for p in parts]
        got = group.link_queue_round(graphs, hts, t, batches, [p[1] for p in parts], "payload", cost_ps=QC.TIE_COST,
                                     root=world - 1, carry=True)
        assert len(got) == 8
        for k, j in ((0, 0), (1, 1), (3, 2), (4, 3), (5, 4)):  # (the group's tuple has the member after the packet)
            assert np.array_equal(got[k], single[j]) and np.array_equal(got[k], tr[j])
        _same_carried(got[6], want, cur, single[5].iterations)
        for a in single[5]._fields[:9]:
            assert np.array_equal(getattr(got[6], a), getattr(single[5], a)), a
        assert np.array_equal(got[7], single[6])
