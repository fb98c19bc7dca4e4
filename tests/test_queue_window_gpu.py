"""sg_link_queue with its window flag on the card, against tests/queue_window_ref.py: every output
starts from sentinels and is compared bit for bit, the packet tails behind the records included.
test_queue_window_ref_cpu.py qualifies the reference.  Without the feature the bit is ignored and
every record is settled: the horizon tests, the session tests and the window_ns tests all fail."""
import numpy as np
import pytest

import outcomes_cases as OC
import queue_carry_cases as CC
import queue_cases as QC
import queue_drop_cases as DC
import queue_gpu_calls as QG
import queue_ref as QR
import queue_window_cases as WC
import queue_window_ref as WR
from queue_gpu_calls import CARRY, DROP, FORMS, INPUTS, VIEW, _batch, _form, _host_table, _net, _pair, _untouched

pytestmark = pytest.mark.gpu

MAX = QR.MAX
RAW = QR.FIELDS
PACKETS, WINDOW = 0x10, WR.WINDOW
MODES = pytest.mark.parametrize("mode", WC.MODES, ids=WC.MODE_IDS)


def _sentinels(c, drop, packets):
    outs = QG._sentinels(c, RAW, drop)
    if packets:
        for k in QR.RECORD_FIELDS:
            outs[k] = np.full(len(c["enter"]) + c["n_packets"], QC.SENT32 if QR.DTYPES[k] == np.uint32 else QC.SENT64, QR.DTYPES[k])
    return outs


def _arrays(c, H, drop, packets):
    free = np.zeros(len(c["link_off"]) - 1, np.uint64) if c["free_in"] is None else c["free_in"]
    a = dict(c, cost_ps=np.concatenate([c["cost_ps"], c["limit_ns"]]) if drop else c["cost_ps"],
             free_in=free if H is None else np.concatenate([free, np.array([H], np.uint64)]))
    if packets:
        a["enter"] = np.concatenate([c["enter"], c["base"]])
    return a


def _call(ctx, c, H, *, dev, drop=False, packets=False, carry=True, n_records=None, null=()):
    """One sg_link_queue call on a case's arrays, the horizon H behind link_free_in (None: the call
    without the bit), every output starting from sentinels.  (status, outputs)."""
    import torch

    from shadow_amd import _capi

    C = _capi.C
    outs = _sentinels(c, drop, packets)
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

    arrays = _arrays(c, H, drop, packets)
    ip = [None if k in null else ptr(arrays[k]) for k in INPUTS]
    n_in = len(keep)
    op = {k: ptr(outs[k]) for k in RAW}
    if dev:
        torch.cuda.synchronize()
    flags = (_capi.SG_ROUTE_OUT_DEVICE if dev else 0) | (CARRY if carry else 0) | (DROP if drop else 0) | \
        (PACKETS if packets else 0) | (0 if H is None else WINDOW)
    rc = _capi.load().sg_link_queue(ctx.handle, flags, len(c["link_off"]) - 1, ip[0],
                                    len(c["enter"]) if n_records is None else n_records, ip[1], ip[2], ip[3],
                                    c["n_packets"], ip[4], ip[5], *[op[k] for k in RAW])
    if dev:
        torch.cuda.synchronize()
        for a, t in keep[n_in:]:
            if a.size:
                a[...] = t.cpu().numpy().view(a.dtype)
    return rc, outs


def _counters(ctx):
    return int(ctx.read_timer("link_queue_iters")[1]), int(ctx.read_timer("link_queue_active")[1])


def _check(ctx, monkeypatch, c, H, modes=WC.MODES, *, devs=(True, False), forms=FORMS, model=True, want=None):
    """The case at horizon H in every mode, form and array mode against the definition; model: the
    iterations and the records sorted equal the restated loop's."""
    from shadow_amd import _capi

    for drop, packets in modes:
        rc, w = (WR.OK, want) if want is not None else WR.define(c, H, drop, packets)
        assert rc == WR.OK
        counts = None
        if model:
            rc, m = WR.jacobi(c, H, drop, packets)
            assert rc == WR.OK
            counts = (m["iters"], m["active"]) if len(c["enter"]) else None
        for form in forms:
            _form(monkeypatch, form)
            for dev in devs:
                rc, outs = _call(ctx, c, H, dev=dev, drop=drop, packets=packets)
                _capi.check(ctx.handle, rc)
                where = (H, drop, packets, form, "device" if dev else "host")
                for k in RAW:
                    assert outs[k].shape == w[k].shape and np.array_equal(outs[k], w[k]), \
                        f"{k} {where}: {int((outs[k] != w[k]).sum())} of {w[k].size} differ, first at " \
                        f"{int(np.flatnonzero(outs[k] != w[k])[0])}"
                if counts:
                    assert _counters(ctx) == counts, where
                if packets:
                    assert int(ctx.read_timer("link_queue_lost")[1]) == w["lost"], where
    return w


# ---- 1. the hand example and the staircases at every kind of horizon
def test_hand_example(ctx, monkeypatch):
    c = WC.hand()
    w = _check(ctx, monkeypatch, c, 118, modes=[(False, True)])
    assert w["pending"].tolist() == [False, False, True, True, False, False]
    for H in WC.horizons(c, False):
        _check(ctx, monkeypatch, c, H)


@pytest.mark.parametrize("k", CC.STAIRS)
def test_staircase(ctx, monkeypatch, k):
    c = WC.staircase(k)
    for H in WC.horizons(c, False):
        _check(ctx, monkeypatch, c, H, devs=(True,))
    _check(ctx, monkeypatch, c, WC.horizons(c, False)[1], devs=(False,), forms=("scan",))


@MODES
def test_the_whole_range_is_the_unflagged_call(ctx, mode):
    """H = 2^64 - 1: every output equals the call without the bit."""
    drop, packets = mode
    for c in (WC.hand(), OC.random_case(2), OC.by_records(257)):
        for dev in (True, False):
            rc0, plain = _call(ctx, c, None, dev=dev, drop=drop, packets=packets)
            rc1, flagged = _call(ctx, c, MAX, dev=dev, drop=drop, packets=packets)
            assert rc0 == 0 and rc1 == 0
            for k in RAW:
                assert np.array_equal(plain[k], flagged[k]), (k, dev)


def test_a_wait_pushes_a_record_past_the_horizon(ctx, monkeypatch):
    w = _check(ctx, monkeypatch, WC.pushed_past(), 110)
    assert w["pending"].sum() == 1


def test_drops_across_the_horizon(ctx, monkeypatch):
    for c, H, _ in WC.drop_cases():
        _check(ctx, monkeypatch, c, H, modes=[(True, False), (True, True)])


# ---- 2. sizes
def _late(c, n_late, t):
    """The case with n_late more single-record packets on link 0 at times from t on: pending at any
    horizon below t."""
    P, n0 = c["n_packets"], int(c["link_off"][1])
    late = dict(c, link_off=c["link_off"] + np.uint64(n_late), n_packets=P + n_late,
                enter=np.insert(c["enter"], n0, np.arange(t, t + n_late, dtype=np.uint64)),
                packet=np.insert(c["packet"], n0, np.arange(P, P + n_late, dtype=np.uint32)),
                weight=np.concatenate([c["weight"], np.full(n_late, 3, np.uint32)]),
                base=np.concatenate([c["base"], np.full(n_late, 77, np.uint64)]))
    late["link_off"][0] = 0
    return late


@pytest.mark.parametrize("length", CC.SEGMENTS)
def test_active_segment_lengths(ctx, monkeypatch, length):
    """A link whose active segment has exactly `length` records, 40 pending ones behind them."""
    c = _late(OC.with_base(DC.draw_limits(CC.from_lengths([length, 70, 3, 0], 31), 32, limits=(60, 200, MAX))), 40, 10**9)
    big = length > 2049
    w = _check(ctx, monkeypatch, c, 10**8, modes=[(True, True)] if big else [(False, False), (True, True)],
               devs=(True,), model=not big)
    assert w["pending"].sum() == 40 and (~w["pending"][:length + 40]).sum() == length


def test_long_chains_cut_by_the_horizon(ctx, monkeypatch):
    """Chains of 2,049 and 65 records, the horizon across both; with the drop at the long chain's
    first record settled, its 2,048 later records are absent."""
    c = OC.long_chains(False)
    w = _check(ctx, monkeypatch, c, 50 + 7 * 40, modes=[(False, True)], devs=(True,), forms=("scan",))
    first = int(w["pending"].sum())
    assert 2000 < first
    w = _check(ctx, monkeypatch, c, 50 + 7 * 1000, modes=[(False, True)], devs=(True,), forms=("scan",), model=False)
    long_chain = c["packet"] == 0
    assert 0 < w["pending"][long_chain].sum() < 2049 and w["pending"].sum() < first  # (the horizon cuts the long chain)
    c = OC.long_chains(True)
    w = _check(ctx, monkeypatch, c, 400, modes=[(True, True)], devs=(True,), forms=("scan",), model=False)
    assert (w["done"][:len(c["enter"])] == np.uint64(MAX)).sum() >= 2048


def test_hot_link(ctx, monkeypatch):
    c = OC.with_base(CC.hot_link())
    w = _check(ctx, monkeypatch, c, 10000, modes=[(False, True)], devs=(True,), forms=("scan",), model=False)
    assert 1000 < w["pending"].sum() < 9000


@pytest.mark.parametrize("n", (0, 1, 255, 256, 257))
def test_record_counts(ctx, monkeypatch, n):
    c = OC.by_records(n)
    H = WC.horizons(c, True)[1] if n else 5
    _check(ctx, monkeypatch, c, H, forms=("scan",))


@pytest.mark.parametrize("P", (0, 1, 257))
def test_packet_counts(ctx, monkeypatch, P):
    c = OC.by_packets(P)
    H = WC.horizons(c, True)[1] if P else 5
    _check(ctx, monkeypatch, c, H, modes=[(False, True), (True, True)], forms=("scan",))


def test_shuffled_input(ctx, monkeypatch):
    c = OC.random_case(5)
    s, perm = CC.shuffled(c, 9)
    H = WC.horizons(c, True)[2]
    rc, w = WR.define(c, H, True, True)
    n = len(c["enter"])
    moved = dict(w)
    for k in QR.RECORD_FIELDS:
        moved[k] = np.concatenate([w[k][:n][perm], w[k][n:]])
    # (where names a record: its index in the shuffled input)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    where = moved["ahead"][n:].copy()
    lost = where < np.uint32(WR.IN_FLIGHT)
    where[lost] = inv[where[lost].astype(np.int64)]
    moved["ahead"] = np.concatenate([moved["ahead"][:n], where])
    _check(ctx, monkeypatch, s, H, modes=[(True, True)], want=moved, model=False)


# ---- 3. errors: code, pair, precedence, every output untouched
@pytest.mark.parametrize("dev", (True, False), ids=("device", "host"))
def test_argument_errors(ctx, dev):
    from shadow_amd import _capi

    c = WC.hand()
    rc, outs = _call(ctx, c, 118, dev=dev, carry=False, packets=True)  # the bit without the carried form
    assert rc == _capi.SG_ERR_INVALID_ARG and _untouched(outs)
    rc, outs = _call(ctx, c, 118, dev=dev, null=("free_in",))
    assert rc == _capi.SG_ERR_INVALID_ARG and _untouched(outs)
    rc, outs = _call(ctx, c, 118, dev=dev, n_records=2**32 - 2)
    assert rc == _capi.SG_ERR_CAPACITY and _untouched(outs)
    rc, outs = _call(ctx, c, 118, dev=dev, n_records=2**32 - 2, null=("free_in",))  # (the NULL comes first)
    assert rc == _capi.SG_ERR_INVALID_ARG and _untouched(outs)
    rc, outs = _call(ctx, c, 118, dev=dev, null=("packet",))  # (the carried form's own error stays ahead)
    assert rc == _capi.SG_ERR_INVALID_ARG and _untouched(outs)
    bad = dict(c, link_off=np.uint64([0, 2, 1, 6]))
    rc, outs = _call(ctx, bad, 118, dev=dev, packets=True)
    assert rc == _capi.SG_ERR_INVALID_ARG and _pair(ctx) == (1, 0xFFFFFFFF) and _untouched(outs)
    bad = dict(c, packet=np.uint32([1, 0, 0, 9, 2, 1]))
    rc, outs = _call(ctx, bad, 118, dev=dev, packets=True)
    assert rc == _capi.SG_ERR_INVALID_ARG and _pair(ctx) == (1, 1) and _untouched(outs)


def test_time_overflow(ctx):
    """A re-based time reaching 2^64 - 1: the pending record behind a crossing served at the range's end."""
    from shadow_amd import _capi

    c = OC.with_base(CC.carry_overflow(0), 0)
    rc, _ = _call(ctx, c, 2**63, dev=True)
    assert rc == _capi.SG_ERR_TIME_OVERFLOW
    c = OC.with_base(CC.carry_overflow(1), 0)
    rc, outs = _call(ctx, c, 2**63, dev=True)
    assert rc == 0 and outs["done"].tolist() == [MAX - 6, MAX - 1] and outs["ahead"].tolist() == [0, 0xFFFFFFFF]


# ---- 4. a non-blocking stream
def test_non_blocking_stream():
    """The windowed call with the drop rule and the packet pass on a context whose stream is the
    caller's non-blocking stream S: the inputs reach the device on S behind a delay, so a launch or
    a copy on any other stream would read them before they are there."""
    import torch

    import stream_cases as SC
    from shadow_amd import Context, _capi

    C = _capi.C
    c = OC.with_base(DC.draw_limits(CC.random_chains(41, n_links=6, n_packets=700, hops=(1, 4), span=4000), 64, limits=(5, 20, 60)))
    H = 2000
    rc, want = WR.define(c, H, True, True)
    assert rc == WR.OK and 0 < want["pending"].sum() < len(c["enter"]) and want["lost"] > 0
    arrays = _arrays(c, H, True, True)
    S = torch.cuda.Stream()
    sctx = Context(0, stream=S.cuda_stream)
    try:
        outs = _sentinels(c, True, True)
        pin = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(VIEW[a.dtype]).copy()).pin_memory()  # noqa: E731
        h_in = [None if arrays[k] is None else pin(arrays[k]) for k in INPUTS]
        h_out = {k: pin(outs[k]) for k in RAW}
        with torch.cuda.stream(S):
            torch.cuda._sleep(SC.DELAY_CYCLES)
            d_in = [None if t is None else t.to("cuda", non_blocking=True) for t in h_in]
            d_out = {k: t.to("cuda", non_blocking=True) for k, t in h_out.items()}
            ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
            rc = _capi.load().sg_link_queue(sctx.handle, _capi.SG_ROUTE_OUT_DEVICE | CARRY | DROP | PACKETS | WINDOW,
                                            len(c["link_off"]) - 1, ptr(d_in[0]), len(c["enter"]), ptr(d_in[1]), ptr(d_in[2]),
                                            ptr(d_in[3]), c["n_packets"], ptr(d_in[4]), ptr(d_in[5]), *[ptr(d_out[k]) for k in RAW])
            for k in RAW:
                h_out[k].copy_(d_out[k], non_blocking=True)
            S.synchronize()
        _capi.check(sctx.handle, rc)
        for k in RAW:
            assert np.array_equal(h_out[k].numpy().view(outs[k].dtype), want[k]), k
    finally:
        S.synchronize()
        sctx.close()


# ---- 5. re-feeding: raw calls, the session, window_ns
def _same_session(got, want):
    for name in ("wait", "done", "delay", "arrive", "lost", "drop_link", "link_free"):
        assert np.array_equal(got[name], want[name]), name
    for name, v in want["sums"].items():
        assert np.array_equal(got["sums"][name], v), name


@pytest.mark.parametrize("drop", (False, True))
def test_re_feeding_through_raw_calls(ctx, drop):
    """queue_window_ref.SessionRef with the library answering every call."""
    from shadow_amd import _capi

    def solve(c, H, drop):
        c = dict(c, limit_ns=c.get("limit_ns"))
        rc, outs = _call(ctx, c, H, dev=True, drop=drop, packets=True)
        _capi.check(ctx.handle, rc)
        return outs

    for k, seed in ((2, 0), (5, 1), (17, 2)):
        c = OC.random_case(100 + seed)
        whole, got = WC.run_session(c, k, seed, drop, solve)
        _same_session(got, WC.session_want(whole, drop))


def _run_python_session(ctx, c, k, seed, drop):
    """WC.run_session through shadow_amd.LinkQueueSession."""
    import shadow_amd

    whole, rs = WC.rounds(c, k, seed)
    nl = len(c["link_off"]) - 1
    s = shadow_amd.LinkQueueSession(ctx, c["cost_ps"], c["limit_ns"] if drop else None, c["free_in"], n_links=nl)
    n, P = len(c["enter"]), c["n_packets"]
    wait, done = np.full(n, 7, np.uint64), np.full(n, 7, np.uint64)
    delay, arrive = np.full(P, 7, np.uint64), np.full(P, 7, np.uint64)
    lost, dlink = np.zeros(P, bool), np.full(P, -1, np.int64)
    seen_r, seen_p = np.zeros(n, int), np.zeros(P, int)
    pend = []
    for r, (rc, H, _, _) in enumerate(rs + [(None, MAX, None, None)]):
        if rc is None:
            pk, rec = s.flush()
        else:
            pk, rec = s.advance(rc["link_off"], rc["enter"], rc["packet"], rc["weight"], rc["base"], H)
        pend.append(s.pending)
        for rr in np.unique(rec.round):
            m = rec.round == rr
            at = rs[rr][2][rec.record[m]]
            wait[at], done[at] = rec.wait_ns[m], rec.done_ns[m]
            np.add.at(seen_r, at, 1)
        for rr in np.unique(pk.round):
            m = pk.round == rr
            at = rs[rr][3][pk.packet[m]]
            delay[at], arrive[at], lost[at] = pk.delay_ns[m], pk.arrive_ns[m], pk.lost[m]
            dlink[at] = np.where(pk.lost[m], pk.drop_link[m].astype(np.int64), -1)
            np.add.at(seen_p, at, 1)
            assert np.array_equal(pk.arrive_dev.cpu().numpy().view(np.uint64), pk.arrive_ns)
    assert (seen_r == 1).all() and (seen_p == 1).all() and s.pending == 0 and s.in_flight == 0
    sums = s.link_sums
    return whole, dict(wait=wait, done=done, delay=delay, arrive=arrive, lost=lost, drop_link=dlink, link_free=s.link_free,
                       sums=dict(busy=sums["busy_ns"], wait_sum=sums["wait_sum_ns"], wait_max=sums["wait_max_ns"],
                                 drops=sums["drops"])), pend


@pytest.mark.parametrize("drop", (False, True))
def test_session_on_random_instances(ctx, drop):
    for k, seed in ((1, 0), (5, 1), (17, 2)):
        whole, got, _ = _run_python_session(ctx, OC.random_case(100 + seed), k, seed, drop)
        _same_session(got, WC.session_want(whole, drop))


@pytest.mark.parametrize("name", ["tie", "k30"])
def test_session_over_five_rounds_of_a_real_trace(ctx, oracle, name):
    """shadow_amd.LinkQueueSession over a real trace cut into 5 rounds by send time, under the median
    limits: one carried call over the concatenation."""
    r = OC.real_trace(oracle, name)
    whole, got, pend = _run_python_session(ctx, r["case"], 5, 7, True)
    assert max(pend) > 0
    want = WC.session_want(whole, True)
    assert want["lost"].any()
    _same_session(got, want)


@pytest.fixture(scope="module")
def tie(ctx, oracle):
    r = OC.real_trace(oracle, "tie")
    net = _net(r["g"], ctx)
    return dict(r, net=net, tree=net.compute_shortest_path_tree())


def test_window_ns_is_the_carried_round(ctx, tie):
    """PathTree.link_queue_round(carry=True, window_ns=) at the trace's smallest gap and at 16 times
    it: every field of the carried result but the iteration count, and the packet outcomes."""
    t, c = tie["tree"], tie["case"]
    ht, pb = _host_table(tie["hosts"], ctx), _batch(tie["pk"])
    kw = dict(cost_ps=QC.TIE_COST, limit_ns=c["limit_ns"], carry=True, outcomes=c["base"])
    want = t.link_queue_round(ht, pb, tie["status"], "payload", **kw)
    nxt, _, gap, _ = WR._chains(c)
    g_min = min(g for g, k in zip(gap, nxt) if k != WR.NONE)
    for W in (g_min, 16 * g_min):
        got = t.link_queue_round(ht, pb, tie["status"], "payload", window_ns=W, **kw)
        assert len(got) == len(want) and type(got[5]) is type(want[5])
        for f in got[5]._fields:
            if f != "iterations":
                assert np.array_equal(getattr(got[5], f), getattr(want[5], f)), (f, W)
        assert np.array_equal(got[6], want[6])
        for f in ("delay_ns", "arrive_ns", "where", "lost", "drop_link"):
            assert np.array_equal(getattr(got[7], f), getattr(want[7], f)), (f, W)
        assert np.array_equal(got[7].arrive_dev.cpu().numpy(), want[7].arrive_dev.cpu().numpy())


def test_python_horizon(ctx, tie):
    """shadow_amd.link_queue(horizon_ns=) and link_queue_pending on host arrays."""
    import shadow_amd

    c, tr = tie["case"], tie["tr"]
    H = WC.horizons(c, True)[1]
    rc, want = WR.define(c, H, True, True)
    n = len(c["enter"])
    q, pk = shadow_amd.link_queue(ctx, tr[0], tr[3], tr[1], c["weight"], cost_ps=c["cost_ps"], carry=True, limit_ns=c["limit_ns"],
                                  outcomes=c["base"], horizon_ns=H)
    pend = shadow_amd.link_queue_pending(q.wait_ns, q.ahead)
    assert np.array_equal(pend, want["pending"]) and 0 < pend.sum() < n
    assert np.array_equal(q.done_ns, want["done"][:n]) and np.array_equal(q.enter_ns[pend], want["done"][:n][pend])
    assert not (q.dropped & pend).any() and not (q.absent & pend).any()
    assert np.array_equal(pk.where, want["ahead"][n:]) and (pk.where == shadow_amd.WHERE_IN_FLIGHT).any()
    assert not pk.lost[pk.where == shadow_amd.WHERE_IN_FLIGHT].any() and pk.lost.sum() == want["lost"]


def test_session_round_runs_the_trace(ctx, tie):
    """LinkQueueSession.round: the tie round's own device trace, settled up to the middle of its
    carried times and then flushed: the carried, limited result of the round."""
    import types

    import shadow_amd

    c, res = tie["case"], tie["res"]
    n, P = len(c["enter"]), c["n_packets"]
    s = shadow_amd.LinkQueueSession(tie["net"], QC.TIE_COST, c["limit_ns"])
    dl = types.SimpleNamespace(status=tie["status"], deliver_time_ns=c["base"])
    H = WC.horizons(c, True)[1]
    pk1, rec1 = s.round(tie["tree"], _host_table(tie["hosts"], ctx), _batch(tie["pk"]), dl, H)
    assert 0 < s.pending < n and 0 < s.in_flight < P and s.last_horizon == H
    pk2, rec2 = s.flush()
    assert s.pending == 0 and s.in_flight == 0
    wait, done = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for rec in (rec1, rec2):
        assert (rec.round == 0).all()
        wait[rec.record], done[rec.record] = rec.wait_ns, rec.done_ns
    assert len(rec1.record) + len(rec2.record) == n
    assert np.array_equal(wait, res.wait) and np.array_equal(done, res.done)
    rc, _, delay, arrive, where = OC.ref(c, True, True)
    got_delay, got_arrive, got_where = np.zeros(P, np.uint64), np.zeros(P, np.uint64), np.zeros(P, np.uint32)
    for pk in (pk1, pk2):
        got_delay[pk.packet], got_arrive[pk.packet], got_where[pk.packet] = pk.delay_ns, pk.arrive_ns, pk.where
    assert np.array_equal(got_delay, delay) and np.array_equal(got_arrive, arrive) and np.array_equal(got_where, where)
    assert np.array_equal(s.link_free, res.link_free) and np.array_equal(s.link_sums["drops"], res.drops.astype(np.uint64))
    with pytest.raises(ValueError):
        s.advance(c["link_off"], c["enter"], c["packet"], c["weight"], c["base"], 5)  # (the horizon went back)


def test_link_queue_device_horizon(ctx, tie):
    """NetworkGraph.link_queue_device(horizon_ns=) passes the bit and the horizon through."""
    import torch

    c = tie["case"]
    H = WC.horizons(c, True)[1]
    rc, want = WR.define(c, H, True, True)
    up = lambda a: torch.from_numpy(a.view(VIEW[a.dtype]).copy()).cuda()  # noqa: E731
    d = {k: up(v) for k, v in _arrays(c, None, False, True).items() if k in ("link_off", "enter", "packet", "weight", "cost_ps")}
    outs = {k: up(v) for k, v in _sentinels(c, True, True).items()}
    torch.cuda.synchronize()
    tie["net"].link_queue_device(d["link_off"].data_ptr(), len(c["packet"]), d["enter"].data_ptr(), d["packet"].data_ptr(),
                                 d["weight"].data_ptr(), c["n_packets"], d["cost_ps"].data_ptr(), 0,
                                 wait_ptr=outs["wait"].data_ptr(), done_ptr=outs["done"].data_ptr(),
                                 ahead_ptr=outs["ahead"].data_ptr(), link_free_ptr=outs["link_free"].data_ptr(),
                                 busy_ptr=outs["busy"].data_ptr(), wait_max_ptr=outs["wait_max"].data_ptr(),
                                 wait_sum_ptr=outs["wait_sum"].data_ptr(), ahead_max_ptr=outs["ahead_max"].data_ptr(),
                                 carry=True, limit_ns=c["limit_ns"], outcomes=True, horizon_ns=H)
    torch.cuda.synchronize()
    for k in RAW:
        assert np.array_equal(outs[k].cpu().numpy().view(want[k].dtype), want[k]), k


# ---- 6. the guard: without the bit the carried call is what it was
@MODES
def test_the_unflagged_call_stands(ctx, monkeypatch, mode):
    drop, packets = mode
    c = OC.random_case(3)
    want, _ = OC.want(c, True, drop)
    n = len(c["enter"])
    for form in FORMS:
        _form(monkeypatch, form)
        rc, outs = _call(ctx, c, None, dev=True, drop=drop, packets=packets)
        assert rc == 0
        for k in RAW:
            w = want[k] if packets or k not in QR.RECORD_FIELDS else want[k][:n]
            assert np.array_equal(outs[k], w), k
