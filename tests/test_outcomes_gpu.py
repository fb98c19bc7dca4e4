"""sg_link_queue with its packets flag on the card, against tests/outcomes_ref.py over the queue
references: every output starts from sentinels and is compared bit for bit, the packet tails behind
the records included.  test_outcomes_ref_cpu.py qualifies the cases.  Without the feature the flag
is ignored and the tails keep their sentinels: the hand example, the real traces, the wire test and
the Python forms all fail."""
import numpy as np
import pytest

import group_trace_cases as GC
import outcomes_cases as OC
import outcomes_ref as OR
import queue_carry_cases as CC
import queue_cases as QC
import queue_drop_cases as DC
import queue_drop_ref as DR
import queue_gpu_calls as QG
import queue_ref as QR
import trace_ref as XR
from queue_gpu_calls import CARRY, DROP, FORMS, INPUTS, VIEW, _batch, _form, _host_table, _net, _pair, _untouched

pytestmark = pytest.mark.gpu

MAX = QR.MAX
RAW = QR.FIELDS
PACKETS = OR.PACKETS
MODES = pytest.mark.parametrize("mode", OC.MODES, ids=OC.MODE_IDS)


def _sentinels(c, names, drop, packets=True):
    """queue_gpu_calls._sentinels, the per-record outputs with the packets behind the records."""
    outs = QG._sentinels(c, names, drop)
    if packets:
        for k in set(QR.RECORD_FIELDS) & set(outs):
            outs[k] = np.full(len(c["enter"]) + c["n_packets"], QC.SENT32 if QR.DTYPES[k] == np.uint32 else QC.SENT64, QR.DTYPES[k])
    return outs


def _arrays(c, drop, packets=True):
    a = dict(c, cost_ps=np.concatenate([c["cost_ps"], c["limit_ns"]]) if drop else c["cost_ps"])
    if packets:
        a["enter"] = np.concatenate([c["enter"], c["base"]])
    return a


def _call(ctx, c, names=RAW, *, dev, carry, drop, packets=True, n_records=None, null=()):
    """One sg_link_queue call with the packets flag on a case's arrays, base behind enter's records,
    the outputs `names` starting from sentinels.  null: inputs passed as NULL.  (status, outputs)."""
    import torch

    from shadow_amd import _capi

    C = _capi.C
    outs = _sentinels(c, names, drop, packets)
    keep = []

    def ptr(a):
        if a is None:
            return None
        if not dev:
            keep.append((a, a if a.size else np.zeros(1, a.dtype)))
            return C.c_void_p(keep[-1][1].ctypes.data)
        t = torch.from_numpy(np.ascontiguousarray(a).view(VIEW[a.dtype]).copy() if a.size else np.zeros(1, VIEW[a.dtype])).cuda()
        keep.append((a, t))
        return C.c_void_p(t.data_ptr())

    arrays = _arrays(c, drop, packets)
    ip = [None if k in null else ptr(arrays[k]) for k in INPUTS]
    n_in = len(keep)
    op = {k: ptr(outs[k]) if k in outs else None for k in RAW}
    if dev:
        torch.cuda.synchronize()
    flags = (_capi.SG_ROUTE_OUT_DEVICE if dev else 0) | (CARRY if carry else 0) | (DROP if drop else 0) | \
        (PACKETS if packets else 0)
    rc = _capi.load().sg_link_queue(ctx.handle, flags, len(c["link_off"]) - 1, ip[0],
                                    len(c["enter"]) if n_records is None else n_records, ip[1], ip[2], ip[3],
                                    c["n_packets"], ip[4], ip[5], *[op[k] for k in RAW])
    if dev:
        torch.cuda.synchronize()
        for a, t in keep[n_in:]:
            if a.size:
                a[...] = t.cpu().numpy().view(a.dtype)
    return rc, outs


def _lost(ctx):
    t = ctx.read_timer("link_queue_lost")
    return int(t[1]), int(t[2])


def _check(ctx, monkeypatch, c, modes=OC.MODES, *, devs=(True, False), forms=FORMS, names=RAW):
    """The case in every mode, form and array mode against the reference, the lost counter too."""
    from shadow_amd import _capi

    for carry, drop in modes:
        want, lost = OC.want(c, carry, drop)
        for form in forms:
            _form(monkeypatch, form)
            for dev in devs:
                rc, outs = _call(ctx, c, names, dev=dev, carry=carry, drop=drop)
                _capi.check(ctx.handle, rc)
                where = (carry, drop, form, "device" if dev else "host")
                for k in names:
                    w = want[k]
                    assert outs[k].shape == w.shape and np.array_equal(outs[k], w), \
                        f"{k} {where}: {int((outs[k] != w).sum())} of {w.size} differ, first at {int(np.flatnonzero(outs[k] != w)[0])}"
                assert _lost(ctx) == (lost, c["n_packets"]), where


# ---- 1. the header's example
def test_hand_example(ctx, monkeypatch):
    c, carried, first = OC.hand()
    n = len(c["enter"])
    for carry, (where, delay) in ((True, carried), (False, first)):
        rc, outs = _call(ctx, c, dev=True, carry=carry, drop=True)
        assert rc == 0
        assert outs["ahead"][n:].tolist() == where and outs["wait"][n:].tolist() == delay
        assert outs["done"][n:].tolist() == [MAX if w < OR.ARRIVED else d for w, d in zip(where, delay)]
    _check(ctx, monkeypatch, c)


# ---- 2. record and packet counts, chains, drops
@pytest.mark.parametrize("n", OC.RECORDS)
def test_record_counts(ctx, monkeypatch, n):
    c = OC.by_records(n)
    _check(ctx, monkeypatch, c)
    if n in (1, 257):
        _check(ctx, monkeypatch, OC.with_empty(c)[0], forms=("scan",))


@pytest.mark.parametrize("P", OC.PACKETS)
def test_packet_counts(ctx, monkeypatch, P):
    """Routes of 1 to 4 links with link_free_in; then no record at all behind P packets."""
    c = OC.by_packets(P)
    _check(ctx, monkeypatch, c)
    e = CC.build(6, [[] for _ in range(P)], np.full(P, 3, np.uint32), [1000] * 6)
    _check(ctx, monkeypatch, OC.with_base(e), forms=("scan",))


@pytest.mark.parametrize("cut", [False, True], ids=["whole", "cut"])
def test_long_chains(ctx, monkeypatch, cut):
    """Chains of 2,049 and 65 records: first order 2,049 adds into one cell; cut at packet 0's
    first link, one dropped record and 2,048 absent (carried) or not counted (first order)."""
    _check(ctx, monkeypatch, OC.long_chains(cut))


@pytest.mark.parametrize("which", ["all", "none", "last", "shuffled"])
def test_drops(ctx, monkeypatch, which):
    c = dict(all=OC.all_dropped, none=OC.none_dropped, last=OC.last_hop_drop, shuffled=lambda: OC.shuffled(OC.random_case(11)))[which]()
    _check(ctx, monkeypatch, c)


INDEX_CASES = dict(hand=lambda: OC.hand()[0], ties=OC.ties, records=lambda: OC.with_empty(OC.by_records(257))[0],
                   tiles=lambda: OC.by_records(OC.RECORDS[-1]), cut=lambda: OC.long_chains(True), all=OC.all_dropped,
                   shuffled=lambda: OC.shuffled(OC.random_case(11)))


@pytest.mark.parametrize("which", list(INDEX_CASES))
def test_first_order_through_the_index(ctx, monkeypatch, which):
    """SG_LINK_QUEUE_PACKETS_INDEX = 1: the first-order pass over every packet's sorted list of records gives
    the same bits as the pass with atomics, equal enter times at a drop included."""
    c = INDEX_CASES[which]()
    _check(ctx, monkeypatch, c, OC.MODES[::2], forms=("scan",))  # (ties: first order only, and the default form here)
    monkeypatch.setenv("SG_LINK_QUEUE_PACKETS_INDEX", "1")
    ctx.enable_timers(True)
    try:
        before = ctx.read_timer("link_queue_index")[1]
        _check(ctx, monkeypatch, c, OC.MODES[::2], forms=("scan",))
        assert ctx.read_timer("link_queue_index")[1] > before  # (the form was taken)
    finally:
        ctx.enable_timers(False)


# ---- 3. values
@MODES
def test_base_values(ctx, monkeypatch, mode):
    """Base 0 and around 2^63; base + delay = 2^64 - 2 is legal, 2^64 - 1 the error, naming a record
    of that packet; a packet without a record keeps a base of 2^64 - 1."""
    from shadow_amd import _capi

    c = OC.random_case(5)
    P = c["n_packets"]
    _check(ctx, monkeypatch, OC.with_base(c, 0), (mode,), forms=("scan",))
    _check(ctx, monkeypatch, OC.with_base(c, np.uint64(1 << 63) - np.uint64(5) + np.arange(P, dtype=np.uint64)), (mode,),
           forms=("scan",))
    e, empty = OC.with_empty(c)
    base = e["base"].copy()
    base[list(empty)] = [MAX, 0, MAX]
    _check(ctx, monkeypatch, dict(e, base=base), (mode,), forms=("scan",))
    legal, p = OC.edge_base(c, *mode, 1)
    _check(ctx, monkeypatch, legal, (mode,))
    over, _ = OC.edge_base(c, *mode, 0)
    rc, recs = OC.ref(over, *mode)[:2]
    assert rc == QR.TIME_OVERFLOW
    off = c["link_off"].astype(np.int64)
    for form, index in ((FORMS[0], "0"), (FORMS[1], "0"), (FORMS[0], "1")):
        _form(monkeypatch, form)
        monkeypatch.setenv("SG_LINK_QUEUE_PACKETS_INDEX", index)
        for dev in (True, False):
            rc, _ = _call(ctx, over, dev=dev, carry=mode[0], drop=mode[1])
            assert rc == _capi.SG_ERR_TIME_OVERFLOW, (form, dev)
            lk, at = _pair(ctx)
            assert lk < len(off) - 1 and int(off[lk]) + at in recs, (form, index, dev, lk, at)


# ---- 4. existing arguments
@MODES
def test_output_subsets(ctx, monkeypatch, mode):
    """No per-link output taken, and each one alone beside the three per-record ones."""
    c = OC.by_packets(257, seed=9)
    assert c["free_in"] is not None
    _check(ctx, monkeypatch, c, (mode,), names=QR.RECORD_FIELDS)
    for k in RAW[3:]:
        _check(ctx, monkeypatch, c, (mode,), names=QR.RECORD_FIELDS + (k,), devs=(True,), forms=("scan",))


@MODES
def test_identity(ctx, monkeypatch, mode):
    """With the bit the first n_records entries and every per-link array equal the call without it."""
    c = OC.random_case(17)
    n = len(c["enter"])
    carry, drop = mode
    for form in FORMS:
        _form(monkeypatch, form)
        for dev in (True, False):
            rc0, plain = _call(ctx, c, dev=dev, carry=carry, drop=drop, packets=False)
            rc1, outs = _call(ctx, c, dev=dev, carry=carry, drop=drop)
            assert rc0 == rc1 == 0
            for k in RAW:
                assert np.array_equal(outs[k][:n] if k in QR.RECORD_FIELDS else outs[k], plain[k]), (k, form, dev)


# ---- 5. errors
@pytest.mark.parametrize("dev", [True, False], ids=["device", "host"])
@MODES
def test_argument_errors(ctx, dev, mode):
    from shadow_amd import _capi

    carry, drop = mode
    c = OC.random_case(2)
    rc, outs = _call(ctx, c, dev=dev, carry=carry, drop=drop, null=("packet", "weight"))
    assert rc == _capi.SG_ERR_INVALID_ARG and _untouched(outs)
    for k in QR.RECORD_FIELDS:
        rc, outs = _call(ctx, c, tuple(x for x in RAW if x != k), dev=dev, carry=carry, drop=drop)
        assert rc == _capi.SG_ERR_INVALID_ARG and _untouched(outs), k
    rc, outs = _call(ctx, c, dev=dev, carry=carry, drop=drop, n_records=(1 << 32) - 1)
    assert rc == _capi.SG_ERR_CAPACITY and _untouched(outs)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dev", [True, False], ids=["device", "host"])
@MODES
def test_data_errors(ctx, monkeypatch, dev, form, mode):
    """A bad link_off before a bad packet index before an arrival past the range, each with the pair
    it has without the bit; a bad packet index is found without weights too."""
    from shadow_amd import _capi

    _form(monkeypatch, form)
    carry, drop = mode
    c, _ = OC.edge_base(OC.random_case(5), carry, drop, 0)
    off = c["link_off"].astype(np.int64)
    pk = c["packet"].copy()
    i = int(off[2]) + 1
    pk[[i, i + 3]] = c["n_packets"]
    bad_off = c["link_off"].copy()
    bad_off[3] = bad_off[2] - np.uint64(1)
    rc, _ = _call(ctx, dict(c, packet=pk, link_off=bad_off), dev=dev, carry=carry, drop=drop)
    assert rc == _capi.SG_ERR_INVALID_ARG and _pair(ctx) == (2, 0xFFFFFFFF)
    for weight in (c["weight"], None):
        rc, _ = _call(ctx, dict(c, packet=pk, weight=weight), dev=dev, carry=carry, drop=drop)
        assert rc == _capi.SG_ERR_INVALID_ARG and _pair(ctx) == (2, 1), (weight is None, _pair(ctx))
    # a record's own overflow comes first: link 0 is free only at the end of time
    free = np.zeros(len(off) - 1, np.uint64)
    free[0] = np.uint64(MAX - 1)
    k = dict(c, free_in=free, limit_ns=DR.unlimited(len(off) - 1), cost_ps=np.full(len(off) - 1, 1000, np.uint64),
             weight=np.maximum(c["weight"], 5).astype(np.uint32))
    assert OC.queue_ref(k, carry, drop)[0] == QR.TIME_OVERFLOW
    rc, _ = _call(ctx, k, dev=dev, carry=carry, drop=drop)
    assert rc == _capi.SG_ERR_TIME_OVERFLOW and (carry or _pair(ctx) == (0, 0))


# ---- 6. a non-blocking stream
def test_non_blocking_stream():
    """The flagged carried call with the drop rule on a context whose stream is the caller's
    non-blocking stream S: the inputs reach the device on S behind a 30 ms delay, so a launch or a
    copy of the packet pass on any other stream would read them, or the record outputs, before
    they are there; the outputs are read back on S."""
    import torch

    import stream_cases as SC
    from shadow_amd import Context, _capi

    C = _capi.C
    c = OC.with_base(DC.draw_limits(CC.random_chains(41, n_links=6, n_packets=700, hops=(1, 4), span=4000), 64, limits=(5, 20, 60)))
    want, lost = OC.want(c, True, True)
    assert 0 < lost < 700
    arrays = _arrays(c, True)
    S = torch.cuda.Stream()
    sctx = Context(0, stream=S.cuda_stream)
    try:
        for flags in (CARRY | DROP, DROP):
            if flags == DROP:
                want, lost = OC.want(c, False, True)
            outs = _sentinels(c, RAW, True)
            pin = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(VIEW[a.dtype]).copy()).pin_memory()  # noqa: E731
            h_in = [None if arrays[k] is None else pin(arrays[k]) for k in INPUTS]
            h_out = {k: pin(outs[k]) for k in RAW}
            with torch.cuda.stream(S):
                torch.cuda._sleep(SC.DELAY_CYCLES)
                d_in = [None if t is None else t.to("cuda", non_blocking=True) for t in h_in]
                d_out = {k: t.to("cuda", non_blocking=True) for k, t in h_out.items()}
                ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
                rc = _capi.load().sg_link_queue(sctx.handle, _capi.SG_ROUTE_OUT_DEVICE | flags | PACKETS, len(c["link_off"]) - 1,
                                                ptr(d_in[0]), len(c["enter"]), ptr(d_in[1]), ptr(d_in[2]), ptr(d_in[3]),
                                                c["n_packets"], ptr(d_in[4]), ptr(d_in[5]), *[ptr(d_out[k]) for k in RAW])
                for k in RAW:
                    h_out[k].copy_(d_out[k], non_blocking=True)
                S.synchronize()
            _capi.check(sctx.handle, rc)
            for k in RAW:
                assert np.array_equal(h_out[k].numpy().view(outs[k].dtype), want[k]), (k, flags)
            assert _lost(sctx) == (lost, 700)
    finally:
        S.synchronize()
        sctx.close()


# ---- 7. real traces through the Python surface
def _same_outcomes(got, c, carry, drop, dev=False):
    rc, _, delay, arrive, where = OC.ref(c, carry, drop)
    assert rc == QR.OK and type(got).__name__ == "PacketOutcomes"
    for x, w in ((got.delay_ns, delay), (got.arrive_ns, arrive), (got.where, where)):
        assert x.dtype == w.dtype and np.array_equal(x, w)
    lost = where < OR.ARRIVED
    assert got.lost.dtype == np.bool_ and np.array_equal(got.lost, lost)
    link = np.full(len(where), 0xFFFFFFFF, np.uint32)
    link[lost] = np.searchsorted(c["link_off"], where[lost].astype(np.uint64), side="right") - 1
    assert got.drop_link.dtype == np.uint32 and np.array_equal(got.drop_link, link)
    if dev:
        assert np.array_equal(got.arrive_dev.cpu().numpy().view(np.uint64), arrive)
    else:
        assert got.arrive_dev is None
    return lost


@pytest.fixture(scope="module")
def tie(ctx, oracle):
    r = OC.real_trace(oracle, "tie")
    net = _net(r["g"], ctx)
    return dict(r, net=net, tree=net.compute_shortest_path_tree())


def test_path_tree_round(ctx, tie, monkeypatch):
    """The tie round through PathTree.link_queue_round(outcomes=): first order and carried under the
    median limits, base times as an array and as a device tensor; and without the keyword the
    tuples are what they were."""
    import torch

    t, tr, c = tie["tree"], tie["tr"], tie["case"]
    ht, pb = _host_table(tie["hosts"], ctx), _batch(tie["pk"])
    kw = dict(cost_ps=QC.TIE_COST, limit_ns=c["limit_ns"])
    base_dev = torch.from_numpy(c["base"].view(np.int64)).cuda()
    for form in FORMS:
        _form(monkeypatch, form)
        got = t.link_queue_round(ht, pb, tie["status"], "payload", carry=True, outcomes=c["base"], **kw)
        assert len(got) == 8 and all(np.array_equal(a, b) for a, b in zip(got[:5], tr))
        assert type(got[5]).__name__ == "LinkQueueCarriedDropped" and np.array_equal(got[5].done_ns, tie["res"].done)
        lost = _same_outcomes(got[7], c, True, True, dev=True)
        assert lost.any() and not lost.all()
        got = t.link_queue_round(ht, pb, tie["status"], "payload", outcomes=base_dev, **kw)
        assert len(got) == 7 and type(got[5]).__name__ == "LinkQueueDropped" and len(got[5].wait_ns) == len(tr[1])
        _same_outcomes(got[6], c, False, True, dev=True)
    got = t.link_queue_round(ht, pb, tie["status"], "payload", carry=True, **kw)
    assert len(got) == 7 and type(got[5]).__name__ == "LinkQueueCarriedDropped"
    got = t.link_queue_round(ht, pb, tie["status"], cost_ps=QC.TIE_COST, outcomes=c["base"])
    assert len(got) == 7 and type(got[5]).__name__ == "LinkQueueResult"
    _same_outcomes(got[6], dict(c, weight=None, limit_ns=DR.unlimited(len(c["cost_ps"]))), False, False, dev=True)


@pytest.mark.parametrize("name", ["k04", "k30"])
def test_link_queue_on_host_arrays(ctx, oracle, monkeypatch, name):
    """shadow_amd.link_queue(outcomes=) on two generated graphs' traces, every mode."""
    import shadow_amd

    r = OC.real_trace(oracle, name)
    c, tr = r["case"], r["tr"]
    for carry, drop in OC.MODES:
        got = shadow_amd.link_queue(ctx, tr[0], tr[3], tr[1], c["weight"], cost_ps=c["cost_ps"], carry=carry,
                                    limit_ns=c["limit_ns"] if drop else None, outcomes=c["base"])
        assert isinstance(got, tuple) and len(got) == 2 and len(got[0].wait_ns) == len(tr[1])
        rc, res = OC.queue_ref(c, carry, drop)
        assert np.array_equal(got[0].done_ns, res.done) and np.array_equal(got[0].ahead, res.ahead)
        lost = _same_outcomes(got[1], c, carry, drop)
        assert lost.any() == drop
    plain = shadow_amd.link_queue(ctx, tr[0], tr[3], tr[1], c["weight"], cost_ps=c["cost_ps"])
    assert type(plain).__name__ == "LinkQueueResult"


def test_link_queue_device(ctx, tie):
    """NetworkGraph.link_queue_device(outcomes=True) passes the bit through."""
    import torch

    c = tie["case"]
    want, _ = OC.want(c, True, True)
    up = lambda a: torch.from_numpy(a.view(VIEW[a.dtype]).copy()).cuda()  # noqa: E731
    d = {k: up(v) for k, v in _arrays(c, False).items() if k in ("link_off", "enter", "packet", "weight", "cost_ps")}
    outs = {k: up(v) for k, v in _sentinels(c, RAW, True).items()}
    torch.cuda.synchronize()
    tie["net"].link_queue_device(d["link_off"].data_ptr(), len(c["enter"]), d["enter"].data_ptr(), d["packet"].data_ptr(),
                                 d["weight"].data_ptr(), c["n_packets"], d["cost_ps"].data_ptr(), wait_ptr=outs["wait"].data_ptr(),
                                 done_ptr=outs["done"].data_ptr(), ahead_ptr=outs["ahead"].data_ptr(),
                                 link_free_ptr=outs["link_free"].data_ptr(), busy_ptr=outs["busy"].data_ptr(),
                                 wait_max_ptr=outs["wait_max"].data_ptr(), wait_sum_ptr=outs["wait_sum"].data_ptr(),
                                 ahead_max_ptr=outs["ahead_max"].data_ptr(), carry=True, limit_ns=c["limit_ns"], outcomes=True)
    torch.cuda.synchronize()
    for k in RAW:
        assert np.array_equal(outs[k].cpu().numpy().view(QR.DTYPES[k]), want[k]), k


@pytest.mark.parametrize("world", QC.GROUP_WORLDS)
def test_group_round(ctx, oracle, tie, world):
    """Group.link_queue_round(outcomes=) over 1 and 3 members on one device: bit-equal to the single
    call on the members' batches concatenated."""
    from test_group_trace_gpu import members

    g, hosts, t = tie["g"], tie["hosts"], tie["tree"]
    parts = GC.split(hosts, tie["pk"], tie["status"], g["n"], world)
    cat, cstatus, _ = GC.concat(parts)
    lim = tie["case"]["limit_ns"]
    rng = np.random.default_rng(world)
    bases = [np.uint64(OC.BASE0) + rng.integers(0, 10**6, len(p[0]["src"])).astype(np.uint64) for p in parts]
    ht, pb = _host_table(hosts, ctx), _batch(cat)
    single = t.link_queue_round(ht, pb, cstatus, "payload", cost_ps=QC.TIE_COST, carry=True, limit_ns=lim,
                                outcomes=np.concatenate(bases))
    tr = single[:5]
    c = OC.with_base(DC.with_limits(CC.case(tr[0], tr[3], tr[1], cat["payload"], np.full(XR.n_links(g), QC.TIE_COST, np.uint64)), lim),
                     np.concatenate(bases))
    lost = _same_outcomes(single[7], c, True, True, dev=True)
    assert lost.any()
    with members(world) as (ctxs, group, keep):
        graphs = [keep(_net(g, x)) for x in ctxs]
        hts = [keep(_host_table(hosts, x)) for x in ctxs]
        batches = [_batch(p[0]) for p in parts]
        for carry in (True, False):
            got = group.link_queue_round(graphs, hts, t, batches, [p[1] for p in parts], "payload", cost_ps=QC.TIE_COST,
                                         root=world - 1, carry=carry, limit_ns=lim, outcomes=bases)
            one = single if carry else t.link_queue_round(ht, pb, cstatus, "payload", cost_ps=QC.TIE_COST, limit_ns=lim,
                                                          outcomes=np.concatenate(bases))
            assert len(got) == len(one) + 1 and type(got[-1]).__name__ == "PacketOutcomes"
            for a in got[-1]._fields[:-1]:
                assert np.array_equal(getattr(got[-1], a), getattr(one[-1], a)), (a, carry)
            assert np.array_equal(got[-1].arrive_dev.cpu().numpy(), one[-1].arrive_dev.cpu().numpy())
            assert np.array_equal(got[6].done_ns, one[5].done_ns)


# ---- 8. a round under link rates, end to end
def test_round_under_link_rates(ctx, oracle, tie):
    """deliver_round, link_queue_round(carry, median limits, outcomes=deliveries), PacketWire.push
    with the resulting times, pop(NEVER): one event per delivered packet the queues did not drop, at
    its reference arrival, in EventQueue order; the count after the pop is exact.  A plain push of
    the same round still gives the delivery's own times."""
    import torch

    from shadow_amd.wire import PacketWire
    from shadow_amd.worker import DeviceTable, PacketBatch, deliver_round
    from test_wire_gpu import _same_pop
    from wire_ref import NEVER, WireRef

    import link_round_cases as RC

    g, hosts, pk, t = tie["g"], tie["hosts"], tie["pk"], tie["tree"]
    nodes = np.arange(g["n"], dtype=np.uint32)
    rc, lat, loss, _ = oracle.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], nodes,
                                             rows=(0, g["n"]), threads=4)
    assert rc == 0
    table = DeviceTable(torch.from_numpy(lat.view(np.int64).ravel()).cuda(), torch.from_numpy(loss.ravel()).cuda(), g["n"])
    ht = _host_table(hosts, ctx)
    pb = PacketBatch.from_numpy(pk["src"], pk["dst_ip"], pk["payload"], pk["send_time"])
    P = len(pk["src"])
    out = deliver_round(ht, table, pb, RC.ROUND_END, 2**63, 0, ctx=ctx)
    dl = out.to_numpy(P)
    assert 0 < dl["delivered"] < P
    # the reference: the delivered packets' trace, the carried result under the median limits
    tr = XR.trace(g, t.nodes, (0, g["n"]), t.pred, t.latency_ns, hosts, pk, dl["status"])
    c = CC.case(tr[0], tr[3], tr[1], pk["payload"], np.full(XR.n_links(g), QC.TIE_COST, np.uint64))
    rc, _, unl = CC.ref(c)[:3]
    assert rc == QR.OK
    c = OC.with_base(DC.with_limits(c, DR.median_limits(c["link_off"], unl.wait)), dl["deliver_time"])
    rc, _, delay, arrive, where = OC.ref(c, True, True)
    assert rc == QR.OK
    delivered = dl["status"] == RC.DELIVERED
    lost = where < OR.ARRIVED
    assert (lost & delivered).any() and (delivered & ~lost & (delay > 0)).any() and not lost[~delivered].any()

    got = t.link_queue_round(ht, pb, out, "payload", cost_ps=QC.TIE_COST, carry=True, limit_ns=c["limit_ns"], outcomes=out)
    oc = got[-1]
    assert np.array_equal(oc.arrive_ns, arrive) and np.array_equal(oc.where, where)
    length = torch.from_numpy((pk["payload"] + 28).astype(np.uint32).view(np.int32)).cuda()
    w, ref = PacketWire(len(hosts["ip"]), P, 10**6, 16, ctx=ctx), WireRef()
    w.push(pb, out, length, id_base=100, deliver_time_ns=oc.arrive_dev)
    assert w.count == P
    order = dl["dst_order"].astype(np.int64)
    host = np.repeat(np.arange(len(dl["dst_offsets"]) - 1), np.diff(dl["dst_offsets"].astype(np.int64)))
    keep = ~lost[order]
    p = order[keep]
    ref.add(host=host[keep], time_ns=arrive[p], src_host=pk["src"][p], event_id=dl["event_id"][p], packet=100 + p,
            len=pk["payload"][p] + 28)
    assert len(ref) == int((delivered & ~lost).sum())
    want, nxt = ref.pop(NEVER)
    _same_pop(w.pop(NEVER), want, nxt)
    assert w.count == 0 and nxt == NEVER
    # the plain push
    ref.push(dl, pk["src"], pk["payload"] + 28, id_base=100)
    w.push(pb, out, length, id_base=100)
    want, nxt = ref.pop(NEVER)
    assert len(want["host"]) == dl["delivered"]
    _same_pop(w.pop(NEVER), want, nxt)
    assert w.count == 0
