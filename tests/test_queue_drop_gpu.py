"""Link queues with finite buffers on the card (sg_link_queue with its drop flag, and limit_ns= of
shadow_amd.link_queue, NetworkGraph.link_queue_device, PathTree.link_queue_round and
Group.link_queue_round) against tests/queue_drop_ref.py.

Every output starts from sentinel values and is compared with np.array_equal; unless a test says
otherwise each case runs in host and in device mode and in both forms (the busy periods walked in
parallel and, under SG_LINK_QUEUE_SERIAL = 1, the lane per link).  First order the reference is the
plain loop (queue_drop_cases.fast, the same loop with `ahead` by bisection, for the large cases);
carried it is the event-driven simulation, and the fixed-point loop gives the iteration counts.
Inputs: tests/queue_drop_cases.py; test_queue_drop_ref_cpu.py qualifies them."""
import functools

import numpy as np
import pytest

import group_trace_cases as GC
import link_cases as LC
import queue_carry_cases as CC
import queue_cases as QC
import queue_drop_cases as DC
import queue_drop_ref as DR
import queue_gpu_calls as QG
import queue_ref as QR
import sweep_cases as WC
import trace_cases as XC
import trace_ref as XR
from queue_gpu_calls import (CARRY, DROP, FORMS, INPUTS, PY_FIELDS, VIEW, _batch, _check_calls, _form, _host_table, _net, _pair,
                             _untouched, ctx_error)

pytestmark = pytest.mark.gpu

MAX = DR.MAX
RAW = QR.FIELDS  # the call's eight output arrays; busy and ahead_max have two entries per link
_call = functools.partial(QG._call, drop=True)
_sentinels = functools.partial(QG._sentinels, drop=True)


def raw(want):
    """A queue_drop_ref.Result as the call's eight arrays."""
    out = {k: getattr(want, k) for k in RAW}
    out["busy"] = np.concatenate([want.busy, want.refused])
    out["ahead_max"] = np.concatenate([want.ahead_max, want.drops])
    return out


def _check(ctx, monkeypatch, c, want=None, *, carry=False, devs=(True, False), forms=FORMS, names=RAW, iters=None):
    """The case in every mode and form against the reference; iters: the iterations every carried
    call must have taken."""
    if want is None:
        if carry:
            rc, _, want, _, _ = DC.ref_carried(c)
        else:
            rc, _, want = DC.ref(c)
        assert rc == DR.OK
    _check_calls(ctx, monkeypatch, c, raw(want), names, carry=carry, drop=True, devs=devs, forms=forms, iters=iters)
    return want


def _mixed(res):
    """Records dropped, served with a wait and served without."""
    served, dropped, _ = DR.states(res)
    return bool(dropped.any() and (res.wait[served] > 0).any() and (res.wait[served] == 0).any())


# ---- 1. the definition's own example
def test_hand_example(ctx, monkeypatch):
    """A is dropped on link 0 and absent on link 1, where C is served at once; D is dropped on
    link 2 behind the carried B, and the first-order flagged call serves it.  Fails where the flag
    is ignored."""
    c, want, _, first = DC.hand()
    _check(ctx, monkeypatch, c, want, carry=True, iters=2)
    _check(ctx, monkeypatch, c, first)
    assert not np.array_equal(want.wait, first.wait)


# ---- 2. busy periods against the tiers and the tile edges
def test_packed_periods(ctx, monkeypatch):
    """Every period length alone on its link (1, 2, around 32 where a lane hands over to a wave,
    around 64 and 2 x 64 + 32 where a wave loads again, around a tile and past three), empty links
    between; a free time per link within 50 ns of the first arrival."""
    c = DC.periods(DC.packed_periods(), 21, 60, free=50)
    want = _check(ctx, monkeypatch, c, DC.fast(c))
    assert _mixed(want) and np.array_equal(np.flatnonzero(DC.period_heads(c)), c["link_off"][1:-1:2].astype(np.int64))


@pytest.mark.parametrize("shift", range(1, 10))
def test_shifted_periods(ctx, monkeypatch, shift):
    """The same lengths on one link behind 1 .. 9 one-record periods: every period meets the
    loads' and the tiles' edges that many records later."""
    c = DC.periods(DC.shifted_periods(shift), 30 + shift, (60, 25)[shift % 2], touch=shift % 3 == 0)
    want = _check(ctx, monkeypatch, c, DC.fast(c), devs=(True,))
    assert _mixed(want)


def test_tile_edge_periods(ctx, monkeypatch):
    """Periods that end exactly on a tile edge and periods that start there."""
    c = DC.periods(DC.edge_periods(), 41, 60)
    heads = np.flatnonzero(DC.period_heads(c))
    assert {DC.TILE, 2 * DC.TILE, 3 * DC.TILE, 4 * DC.TILE}.issubset(heads.tolist())
    assert _mixed(_check(ctx, monkeypatch, c, DC.fast(c)))


def test_one_period_of_100000(ctx, monkeypatch):
    """One link, one busy period of 100,000 records (the hot link): a wave walks it."""
    c = DC.periods([[100000]], 42, 60)
    want = _check(ctx, monkeypatch, c, DC.fast(c), devs=(True,))
    assert _mixed(want) and int(want.drops[0]) > 30000
    _check(ctx, monkeypatch, c, want, devs=(False,), forms=("scan",))


def test_every_record_its_own_period(ctx, monkeypatch):
    """5,000 records that each find the unlimited server idle; limit 0 drops none of them."""
    c = DC.periods([[1] * 5000, [], [1] * 3], 43, 0, touch=True)
    want = _check(ctx, monkeypatch, c, DC.fast(c))
    assert not want.drops.any() and not want.wait_max.any()


@pytest.fixture(scope="module")
def second_trip():
    c = DC.periods(DC.mixed_periods(QC.SECOND_TRIP, 44), 45, 60, free=50)
    return c, DC.fast(c)


@pytest.mark.parametrize("form", FORMS)
def test_second_trip(ctx, monkeypatch, second_trip, form):
    """One segment of 2,097,153 records, one past 1,024 tiles, of mixed periods (1 .. 5,000
    records): the unlimited pass's carry kernel loops, the marks' sums take more than one block of
    block sums.  Device mode; the reference is the plain loop."""
    c, want = second_trip
    assert len(c["enter"]) == QC.SECOND_TRIP and _mixed(want)
    _check(ctx, monkeypatch, c, want, devs=(True,), forms=(form,))


# ---- 3. limits, free times, the order given, large values
@pytest.mark.parametrize("limit", [0, 1, 25, 60, MAX])
def test_limits(ctx, monkeypatch, limit):
    c = DC.periods([[1, 40, 2, 300, 70], [], [33, 5]], 51, limit, free=50)
    want = _check(ctx, monkeypatch, c)
    assert bool(want.drops.any()) == (limit != MAX)
    if limit == MAX:  # the identity: the unflagged call's result, the second halves 0
        rc, outs = _call(ctx, c, dev=True, drop=False)
        assert rc == 0 and all(np.array_equal(outs[k], getattr(want, k)) for k in RAW)
        assert not want.refused.any()


def test_limits_per_link(ctx, monkeypatch):
    c = DC.draw_limits(QC.random_trace([0, 70, 300, 1, 2100, 64, 65, 0], 52, free_max=100), 53)
    c["n_packets"] = len(c["weight"])
    assert _mixed(_check(ctx, monkeypatch, c))


def test_all_but_the_first_dropped(ctx, monkeypatch):
    """2,500 records at one instant under limit 0: the first is served, every other one dropped;
    and a link whose first record link_free_in drops (its server is free 61 ns late)."""
    c = DC.with_limits(QC.case([0, 2500, 2505], [1000] * 2500 + [1000, 1010, 1020, 1030, 1200], cost_ps=[5000, 5000],
                               free_in=[0, 1061]), [0, 60])
    c["n_packets"] = 0
    want = _check(ctx, monkeypatch, c)
    served, dropped, _ = DR.states(want)
    assert served[:2500].tolist() == [True] + [False] * 2499 and want.link_free.tolist() == [1005, 1205]
    assert dropped[2500] and not dropped[2501:].any() and want.drops.tolist() == [2499, 1]


def test_unsorted_segments(ctx, monkeypatch):
    """First order the result is a function of the arrays as given."""
    c = DC.draw_limits(QC.random_trace([300, 0, 2100, 65], 54, free_max=100), 55, limits=(5, 20, 60))
    c["n_packets"] = len(c["weight"])
    s, perm = CC.shuffled(c, 56)
    assert not np.array_equal(perm, np.arange(len(perm)))
    want = _check(ctx, monkeypatch, s)
    assert _mixed(want) and not np.array_equal(want.wait, DC.ref(c)[2].wait[perm])


def test_large_values(ctx, monkeypatch):
    """Times near 2^63, services near 2^61 from products past 2^64 (weight 2^31 - 1 at 2^40 ps);
    the unlimited pass saturates at 2^64 - 1 on both links and flags nothing, the limited result
    is clean: a dropped record never overflows."""
    t = 2**63
    s = QR.service(2**31 - 1, 2**40)
    assert s > 2**61 and (2**31 - 1) * 2**40 > 2**64
    enter = [t + 10 * k for k in range(12)] + [100 + k for k in range(70)]
    c = QC.case([0, 12, 82], enter, [0] * 82, [2**31 - 1], [2**40, 10**4], [0, MAX - 25])
    c = DC.with_limits(dict(c, n_packets=1), [s + 100, 50])
    assert DC.ref(DC.with_limits(c, MAX))[0] == DR.TIME_OVERFLOW
    want = _check(ctx, monkeypatch, c)
    assert want.drops.tolist() == [10, 70] and want.link_free.tolist() == [t + 2 * s, MAX - 25]
    # served past 2^64 - 1 is the error it was: the smallest such record
    bad = DC.with_limits(c, [3 * s + 100, 50])
    code, pair, _ = DC.ref(bad)
    assert (code, pair) == (DR.TIME_OVERFLOW, (0, 3))
    for form in FORMS:
        _form(monkeypatch, form)
        for dev in (True, False):
            rc, _ = _call(ctx, bad, dev=dev)
            assert (rc, _pair(ctx)) == (code, pair)


# ---- 4. carried
@pytest.mark.parametrize("seed", range(8))
def test_carried_random(ctx, monkeypatch, seed):
    rng = np.random.default_rng(4000 + seed)
    c = CC.random_chains(100 + seed, n_links=int(rng.integers(2, 9)), n_packets=int(rng.integers(50, 400)),
                         hops=(1, int(rng.integers(2, 7))), span=int(rng.integers(300, 3000)), free_max=(0, 300)[seed % 2])
    c = DC.draw_limits(c, 5000 + seed)
    rc, _, want, _, iters = DC.ref_carried(c, jacobi=True)
    assert rc == DR.OK
    _check(ctx, monkeypatch, c, want, carry=True, iters=iters)


def test_carried_segment_lengths(ctx, monkeypatch):
    """Link segments across the sort's tiers and the scan's tile edges, limits per link."""
    c = DC.draw_limits(CC.from_lengths(CC.SEGMENTS, 4, free_max=500), 61, limits=(0, 20, 60, 200, MAX))
    want = _check(ctx, monkeypatch, c, carry=True)
    served, dropped, absent = DR.states(want)
    assert dropped.any() and absent.any() and (want.wait[served] > 0).any()


@pytest.mark.parametrize("limit", [0, 50, 500])
def test_carried_hot_link(ctx, monkeypatch, limit):
    """One link of 5,000 records behind 50 slow feeders, every buffer alike."""
    c = DC.with_limits(CC.hot_link(), limit)
    want = _check(ctx, monkeypatch, c, carry=True, devs=(True,))
    assert int(want.drops.sum()) == {0: 2689, 50: 954, 500: 4}[limit]


def test_carried_long_chain_cut(ctx, monkeypatch):
    """long_chains with packet 0 dropped on its first link (the link is free only 100 ns after it
    arrives, its buffer holds 60): its 2,048 later records are absent."""
    c = CC.long_chains()
    free = np.zeros(CC.PIECE + 1, np.uint64)
    free[0] = 150
    c = DC.with_limits(dict(c, free_in=free), 60)
    want = _check(ctx, monkeypatch, c, carry=True, devs=(True,))
    _, dropped, absent = DR.states(want)
    assert dropped[c["packet"] == 0].sum() == 1 and absent[c["packet"] == 0].sum() == CC.PIECE


def test_carried_shuffled_input(ctx, monkeypatch):
    c = DC.draw_limits(CC.random_chains(7, n_links=6, n_packets=900, hops=(1, 4), span=5000), 62, limits=(5, 20, 60))
    want = DC.ref_carried(c)[2]
    s, perm = CC.shuffled(c, 8)
    got = _check(ctx, monkeypatch, s, carry=True)
    for k in QR.RECORD_FIELDS:
        assert np.array_equal(getattr(got, k), getattr(want, k)[perm]), k
    assert np.array_equal(got.drops, want.drops) and DR.states(got)[2].any()


# ---- 5. the outputs taken
def test_output_subsets(ctx, monkeypatch):
    """Each output alone (the doubled arrays among them), pairs, unit weights, no record."""
    from shadow_amd import _capi

    c = DC.draw_limits(CC.random_chains(14, n_links=7, n_packets=600, hops=(1, 4), span=4000, free_max=200), 63,
                       limits=(5, 20, 60))
    for carry in (False, True):
        for names in [(k,) for k in RAW] + [("ahead", "ahead_max"), ("wait", "busy"), ("done", "link_free")]:
            _check(ctx, monkeypatch, c, carry=carry, names=names, devs=(True,), forms=("scan",))
        _check(ctx, monkeypatch, c, carry=carry, names=("busy", "ahead_max"), devs=(False,))
    _check(ctx, monkeypatch, dict(c, weight=None))
    _check(ctx, monkeypatch, dict(c, weight=None), carry=True)
    empty = DC.with_limits(dict(QC.case([0, 0, 0, 0], [], [], None, [5, 6, 7], [9, 8, 7]), n_packets=0), [1, 2, 3])
    for dev in (True, False):
        for carry in (False, True):
            rc, outs = _call(ctx, empty, dev=dev, carry=carry)
            assert rc == _capi.SG_OK and outs["link_free"].tolist() == [9, 8, 7]
            assert not outs["busy"].any() and not outs["ahead_max"].any() and not outs["wait_max"].any()
            assert len(outs["busy"]) == len(outs["ahead_max"]) == 6


# ---- 6. errors
@pytest.mark.parametrize("dev", [True, False], ids=["device", "host"])
def test_argument_errors(ctx, dev):
    """With the flag, every output untouched: today's argument errors, a record count past 2^32 -
    2 (SG_ERR_CAPACITY, refused before any array is read), a host-mode bad link_off."""
    from shadow_amd import _capi

    c, _, _, _ = DC.hand()
    for carry in (False, True):
        rc, outs = _call(ctx, c, (), dev=dev, carry=carry)
        assert rc == _capi.SG_ERR_INVALID_ARG and "no output" in ctx_error(ctx)
        rc, outs = _call(ctx, c, dev=dev, carry=carry, n_records=2**32 - 1)
        assert rc == _capi.SG_ERR_CAPACITY and _untouched(outs)
        if not dev:
            rc, outs = _call(ctx, dict(c, link_off=np.uint64([0, 3, 2, 6])), dev=dev, carry=carry)
            assert (rc, _pair(ctx)) == (_capi.SG_ERR_INVALID_ARG, (1, QR.UMAX)) and _untouched(outs)
    rc, outs = _call(ctx, dict(c, packet=None, weight=None), dev=dev, carry=True)
    assert rc == _capi.SG_ERR_INVALID_ARG and _untouched(outs) and "without packet" in ctx_error(ctx)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dev", [True, False], ids=["device", "host"])
def test_data_errors(ctx, monkeypatch, dev, form):
    """A bad link_off; a packet index not below n_weights; two records of one packet at one time
    (carried); a served done, and carried done + gap alone, reaching 2^64 - 1; the precedence
    link_off, packet, twin, overflow; and the dropped record that would have overflowed and does
    not.  Codes and pairs are the reference's."""
    _form(monkeypatch, form)
    c, want, _, first = DC.hand()
    pk = c["packet"].copy()
    pk[[3, 4]] = 4, 7
    twin = np.uint64([100, 102, 107, 126, 100, 118])  # packet 1's records 0 and 4 at one time
    wild = np.uint64([0, 2**40, 4, 6])
    far = dict(free_in=np.uint64([0, 0, MAX - 12]), limit_ns=np.uint64([5, 5, MAX]))
    cases = [dict(c, link_off=wild), dict(c, link_off=wild, packet=pk, enter=twin, **far),
             dict(c, link_off=np.uint64([0, 2, 4, 5]), packet=pk),
             dict(c, packet=pk), dict(c, packet=pk, enter=twin, **far), dict(c, enter=twin), dict(c, enter=twin, **far),
             dict(c, **far), DC.with_limits(CC.carry_overflow(0), MAX)]
    if dev is False:
        cases = cases[3:]  # (a bad host link_off is an argument error: test_argument_errors)
    for bad in cases:
        for carry in (True, False):
            code, pair = (DC.ref_carried(bad) if carry else DC.ref(bad))[:2]
            rc, outs = _call(ctx, bad, dev=dev, carry=carry)
            assert rc == code, (bad, carry, ctx_error(ctx))
            assert code == DR.OK or pair is None or _pair(ctx) == pair, (bad, carry, ctx_error(ctx))
    # the call after an error is a good one
    rc, outs = _call(ctx, c, dev=dev, carry=True)
    assert rc == 0 and all(np.array_equal(outs[k], raw(want)[k]) for k in RAW)
    # dropped, the record that overflowed above does not; nor does a dropped record carry
    near = dict(c, free_in=far["free_in"], limit_ns=np.uint64([5, 5, 5]))
    for carry in (True, False):
        res = (DC.ref_carried(near) if carry else DC.ref(near))[2]
        rc, outs = _call(ctx, near, dev=dev, carry=carry)
        assert rc == 0 and all(np.array_equal(outs[k], raw(res)[k]) for k in RAW)
    cut = DC.with_limits(CC.carry_overflow(0), 5)
    rc, outs = _call(ctx, cut, dev=dev, carry=True)
    assert rc == 0 and outs["wait"].tolist() == [MAX, MAX] and outs["done"].tolist() == [100, MAX]
    ok = DC.with_limits(CC.carry_overflow(1), MAX)
    rc, outs = _call(ctx, ok, dev=dev, carry=True)
    assert rc == 0 and outs["done"].tolist() == [MAX - 6, MAX - 1]


def test_iteration_cap(ctx, monkeypatch):
    from shadow_amd import _capi

    c = DC.with_limits(CC.staircase(6), 5)
    monkeypatch.setenv("SG_LINK_QUEUE_CARRY_ITERS", "1")
    for dev in (True, False):
        rc, outs = _call(ctx, c, dev=dev, carry=True)
        assert (rc, _pair(ctx)) == (_capi.SG_ERR_CAPACITY, (1, QR.UMAX))
    assert DC.ref_carried(c, jacobi=True, cap=1)[:2] == (DR.CAPACITY, (1, QR.UMAX))
    monkeypatch.delenv("SG_LINK_QUEUE_CARRY_ITERS")
    rc, _, want, _, iters = DC.ref_carried(c, jacobi=True)
    _check(ctx, monkeypatch, c, want, carry=True, forms=("scan",), iters=iters)


# ---- 7. a non-blocking stream
def test_non_blocking_stream():
    """The flagged carried call on a context whose stream is the caller's non-blocking stream S:
    the inputs reach the device on S behind a 30 ms delay, so a launch or a copy on any other
    stream would read them before they are there; the outputs are read back on S."""
    import torch

    import stream_cases as SC
    from shadow_amd import Context, _capi

    C = _capi.C
    c = DC.draw_limits(CC.random_chains(41, n_links=6, n_packets=700, hops=(1, 4), span=4000), 64, limits=(5, 20, 60))
    rc, _, res, _, _ = DC.ref_carried(c)
    assert rc == DR.OK and DR.states(res)[1].any() and DR.states(res)[2].any()
    want = raw(res)
    arrays = dict(c, cost_ps=np.concatenate([c["cost_ps"], c["limit_ns"]]))
    S = torch.cuda.Stream()
    sctx = Context(0, stream=S.cuda_stream)
    try:
        outs = _sentinels(c, RAW)
        pin = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(VIEW[a.dtype]).copy()).pin_memory()  # noqa: E731
        h_in = [None if arrays[k] is None else pin(arrays[k]) for k in INPUTS]
        h_out = {k: pin(outs[k]) for k in RAW}
        with torch.cuda.stream(S):
            torch.cuda._sleep(SC.DELAY_CYCLES)
            d_in = [None if t is None else t.to("cuda", non_blocking=True) for t in h_in]
            d_out = {k: t.to("cuda", non_blocking=True) for k, t in h_out.items()}
            ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
            rc = _capi.load().sg_link_queue(sctx.handle, _capi.SG_ROUTE_OUT_DEVICE | CARRY | DROP, len(c["link_off"]) - 1,
                                            ptr(d_in[0]), len(c["enter"]), ptr(d_in[1]), ptr(d_in[2]), ptr(d_in[3]),
                                            c["n_packets"], ptr(d_in[4]), ptr(d_in[5]), *[ptr(d_out[k]) for k in RAW])
            for k in RAW:
                h_out[k].copy_(d_out[k], non_blocking=True)
            S.synchronize()
        _capi.check(sctx.handle, rc)
        for k in RAW:
            assert np.array_equal(h_out[k].numpy().view(outs[k].dtype), want[k]), k
    finally:
        S.synchronize()
        sctx.close()


# ---- 8. real traces through the Python surface
DROP_FIELDS = dict(PY_FIELDS, link_drops="drops", link_refused_ns="refused")


def _same_dropped(got, want, cur=None, iters=None):
    """A LinkQueueDropped or LinkQueueCarriedDropped against the reference."""
    for a, b in DROP_FIELDS.items():
        x, w = getattr(got, a), getattr(want, b)
        assert x.dtype == w.dtype and np.array_equal(x, w), a
    served, dropped, absent = DR.states(want)
    assert got.dropped.dtype == np.bool_ and np.array_equal(got.dropped, dropped)
    if cur is not None:
        assert np.array_equal(got.absent, absent)
        assert got.enter_ns.dtype == np.uint64 and np.array_equal(got.enter_ns, cur)
        assert iters is None or got.iterations == iters


def _limited(c, carried):
    rc, _, unl = (CC.ref(c) if carried else QC.ref(c))[:3]
    assert rc == QR.OK
    return DC.with_limits(c, DR.median_limits(c["link_off"], unl.wait)), unl


@pytest.fixture(scope="module")
def tie(ctx):
    """The tie round, its tree, its trace and the references under queue_cases.TIE_COST with the
    median rule's limits, first order and carried."""
    g = LC.tie_graph()
    hosts, pk, mixed = XC.tie_round()
    net = _net(g, ctx)
    t = net.compute_shortest_path_tree()
    tr = XR.trace(g, t.nodes, (0, g["n"]), t.pred, t.latency_ns, hosts, pk)
    c = CC.case(tr[0], tr[3], tr[1], pk["payload"], np.full(XR.n_links(g), QC.TIE_COST, np.uint64))
    fo, _ = _limited(c, False)
    ca, unl = _limited(c, True)
    rc, _, want, cur, _ = DC.ref_carried(ca)
    assert rc == DR.OK
    return dict(g=g, hosts=hosts, pk=pk, mixed=mixed, net=net, tree=t, tr=tr, case=c, first=fo, first_want=DC.fast(fo),
                carried=ca, want=want, cur=cur, unl=unl)


def test_path_tree_round(ctx, tie, monkeypatch):
    """The tie round through PathTree.link_queue_round(limit_ns=), payload weights, both forms,
    first order and carried; the carried exit is 2^64 - 1 at a dropped or absent hop.  Fails where
    the flag is ignored.  And the guard: without limit_ns both calls give what they gave."""
    t, tr = tie["tree"], tie["tr"]
    ht, pb = _host_table(tie["hosts"], ctx), _batch(tie["pk"])
    want = tie["want"]
    served, dropped, absent = DR.states(want)
    assert dropped.any() and absent.any() and (served & (want.wait < tie["unl"].wait)).any()
    its = set()
    for form in FORMS:
        _form(monkeypatch, form)
        got = t.link_queue_round(ht, pb, None, "payload", cost_ps=QC.TIE_COST, limit_ns=tie["first"]["limit_ns"])
        assert len(got) == 6 and all(np.array_equal(a, b) for a, b in zip(got[:5], tr))
        _same_dropped(got[5], tie["first_want"])
        got = t.link_queue_round(ht, pb, None, "payload", cost_ps=QC.TIE_COST, carry=True, limit_ns=tie["carried"]["limit_ns"])
        assert len(got) == 7 and all(np.array_equal(a, b) for a, b in zip(got[:5], tr))
        _same_dropped(got[5], want, tie["cur"])
        its.add(got[5].iterations)
        exit_ns = tr[4] + (want.done - tr[3])
        exit_ns[~served] = MAX
        assert np.array_equal(got[6], exit_ns)
    assert len(its) == 1
    _check(ctx, monkeypatch, tie["carried"], want, carry=True, forms=("scan",), iters=its.pop())
    _check(ctx, monkeypatch, tie["first"], tie["first_want"], forms=("scan",))
    # the guard
    rc, _, first = QC.ref(tie["case"])
    got = t.link_queue_round(ht, pb, None, "payload", cost_ps=QC.TIE_COST)
    assert len(got) == 6 and type(got[5]).__name__ == "LinkQueueResult"
    for a, b in PY_FIELDS.items():
        assert np.array_equal(getattr(got[5], a), getattr(first, b)), a
    got = t.link_queue_round(ht, pb, None, "payload", cost_ps=QC.TIE_COST, carry=True)
    assert type(got[5]).__name__ == "LinkQueueCarried"
    for a, b in PY_FIELDS.items():
        assert np.array_equal(getattr(got[5], a), getattr(tie["unl"], b)), a
    for carry, ref in ((False, first), (True, tie["unl"])):
        rc, outs = _call(ctx, tie["case"], dev=True, carry=carry, drop=False)
        assert rc == 0 and all(np.array_equal(outs[k], getattr(ref, k)) for k in RAW)


def test_identity(ctx, tie, monkeypatch):
    """Every limit 2^64 - 1: the flagged call equals the unflagged one in every first-half output,
    plain and carried, and the second halves are 0."""
    c = DC.with_limits(tie["case"], MAX)
    nl = len(c["cost_ps"])
    for carry, ref in ((False, QC.ref(c)[2]), (True, tie["unl"])):
        for form in FORMS:
            _form(monkeypatch, form)
            rc, outs = _call(ctx, c, dev=True, carry=carry)
            assert rc == 0
            for k in RAW:
                w = getattr(ref, k)
                assert np.array_equal(outs[k][:len(w)], w), (k, carry, form)
            assert not outs["busy"][nl:].any() and not outs["ahead_max"][nl:].any()


def test_link_queue_device(ctx, tie):
    """NetworkGraph.link_queue_device(limit_ns=): the doubled cost array is built from the
    caller's device costs and the host limits."""
    import torch

    c, want = tie["first"], raw(tie["first_want"])
    up = lambda a: torch.from_numpy(a.view(VIEW[a.dtype]).copy()).cuda()  # noqa: E731
    d = {k: up(c[k]) for k in ("link_off", "enter", "packet", "weight", "cost_ps")}
    outs = {k: up(v) for k, v in _sentinels(c, RAW).items()}
    torch.cuda.synchronize()
    tie["net"].link_queue_device(d["link_off"].data_ptr(), len(c["enter"]), d["enter"].data_ptr(), d["packet"].data_ptr(),
                                 d["weight"].data_ptr(), len(c["weight"]), d["cost_ps"].data_ptr(), wait_ptr=outs["wait"].data_ptr(),
                                 done_ptr=outs["done"].data_ptr(), ahead_ptr=outs["ahead"].data_ptr(),
                                 link_free_ptr=outs["link_free"].data_ptr(), busy_ptr=outs["busy"].data_ptr(),
                                 wait_max_ptr=outs["wait_max"].data_ptr(), wait_sum_ptr=outs["wait_sum"].data_ptr(),
                                 ahead_max_ptr=outs["ahead_max"].data_ptr(), limit_ns=c["limit_ns"])
    torch.cuda.synchronize()
    for k in RAW:
        assert np.array_equal(outs[k].cpu().numpy().view(QR.DTYPES[k]), want[k]), k


@pytest.mark.parametrize("name", ["k04", "k30"])
def test_sweep(ctx, oracle, monkeypatch, name):
    """Two generated graphs, queue_cases.sweep_round, one cost per link drawn from {0, 80, 8,000,
    10^6} ps, payload weights, the median rule's limits: shadow_amd.link_queue(limit_ns=) on the
    reference trace, first order and carried.  Fails where the flag is ignored."""
    import shadow_amd

    c, r = WC.case(name), WC.refs(oracle, name)[0]
    g, n = c["g"], c["g"]["n"]
    pk, status = QC.sweep_round(c)
    tr = XR.trace(g, c["nodes"], (0, n), r["pred"], r["lat"], c["hosts"], pk, status)
    k = CC.case(tr[0], tr[3], tr[1], pk["payload"], QC.sweep_costs(name, XR.n_links(g)))
    fo, _ = _limited(k, False)
    ca, unl = _limited(k, True)
    rc, _, want, cur, iters = DC.ref_carried(ca, jacobi=True)
    assert rc == DR.OK and DR.states(want)[1].any() and DR.states(want)[2].any()
    first = DC.ref(fo)[2]
    for form in FORMS:
        _form(monkeypatch, form)
        got = shadow_amd.link_queue(ctx, tr[0], tr[3], tr[1], pk["payload"], cost_ps=k["cost_ps"], carry=True,
                                    limit_ns=ca["limit_ns"])
        assert type(got).__name__ == "LinkQueueCarriedDropped"
        _same_dropped(got, want, cur, iters)
        got = shadow_amd.link_queue(ctx, tr[0], tr[3], tr[1], pk["payload"], cost_ps=k["cost_ps"], limit_ns=fo["limit_ns"])
        assert type(got).__name__ == "LinkQueueDropped"
        _same_dropped(got, first)


@pytest.mark.parametrize("world", QC.GROUP_WORLDS)
def test_group_round(ctx, tie, world):
    """Group.link_queue_round(limit_ns=) over 1 and 3 members on one device, first order and
    carried: the reference on the members' batches concatenated, and the single call on that
    batch bit for bit."""
    from test_group_trace_gpu import members

    g, hosts, t = tie["g"], tie["hosts"], tie["tree"]
    status = QC.group_status(tie["mixed"])
    parts = GC.split(hosts, tie["pk"], status, g["n"], world)
    cat, cstatus, _ = GC.concat(parts)
    tr = XR.trace(g, t.nodes, (0, g["n"]), t.pred, t.latency_ns, hosts, cat, cstatus)
    c = CC.case(tr[0], tr[3], tr[1], cat["payload"], np.full(XR.n_links(g), QC.TIE_COST, np.uint64))
    ca, _ = _limited(c, True)
    lim = ca["limit_ns"]
    rc, _, want, cur, _ = DC.ref_carried(ca)
    assert rc == DR.OK and DR.states(want)[1].any() and DR.states(want)[2].any()
    ht, pb = _host_table(hosts, ctx), _batch(cat)
    single = t.link_queue_round(ht, pb, cstatus, "payload", cost_ps=QC.TIE_COST, carry=True, limit_ns=lim)
    single1 = t.link_queue_round(ht, pb, cstatus, "payload", cost_ps=QC.TIE_COST, limit_ns=lim)
    _same_dropped(single[5], want, cur)
    _same_dropped(single1[5], DC.fast(ca))
    with members(world) as (ctxs, group, keep):
        graphs = [keep(_net(g, x)) for x in ctxs]
        hts = [keep(_host_table(hosts, x)) for x in ctxs]
        batches = [_batch(p[0]) for p in parts]
        got = group.link_queue_round(graphs, hts, t, batches, [p[1] for p in parts], "payload", cost_ps=QC.TIE_COST,
                                     root=world - 1, carry=True, limit_ns=lim)
        assert len(got) == 8
        for k, j in ((0, 0), (1, 1), (3, 2), (4, 3), (5, 4)):  # (the group's tuple has the member after the packet)
            assert np.array_equal(got[k], single[j]) and np.array_equal(got[k], tr[j])
        _same_dropped(got[6], want, cur, single[5].iterations)
        for a in single[5]._fields[:-1]:
            assert np.array_equal(getattr(got[6], a), getattr(single[5], a)), a
        assert np.array_equal(got[7], single[6])
        got = group.link_queue_round(graphs, hts, t, batches, [p[1] for p in parts], "payload", cost_ps=QC.TIE_COST,
                                     root=world - 1, limit_ns=lim)
        assert len(got) == 7
        for a in single1[5]._fields:
            assert np.array_equal(getattr(got[6], a), getattr(single1[5], a)), a
