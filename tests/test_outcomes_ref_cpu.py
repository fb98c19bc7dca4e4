"""The packet outcomes' definition (outcomes_ref.py) and the cases of test_outcomes_gpu.py, qualified on
the CPU: the header's hand example, the two facts the carried kernel rests on, the first-order rule,
packets without a record, the error rules, the real traces against the host-side fold the feature
replaces, and the flag through the layers."""
import inspect
import os
import re

import numpy as np
import pytest

import outcomes_cases as OC
import outcomes_ref as OR
import queue_drop_ref as DR
import queue_ref as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX = QR.MAX


def test_hand_example():
    c, carried, first = OC.hand()
    for carry, (where, delay) in ((True, carried), (False, first)):
        rc, _, d, a, w = OC.ref(c, carry, True)
        assert rc == QR.OK
        assert w.tolist() == where and d.tolist() == delay
        lost = [x < OR.ARRIVED for x in where]
        assert a.tolist() == [MAX if gone else dl for gone, dl in zip(lost, delay)]  # (base 0)
    # without the drop rule every record is served: A waits 8 on link 0, C 9 behind it on link 1, D 7 behind B on link 2
    rc, _, d, a, w = OC.ref(c, True, False)
    assert w.tolist() == [OR.ARRIVED] * 4 and d.tolist() == [28, 20, 19, 17] and a.tolist() == d.tolist()


@pytest.mark.parametrize("seed", range(36))
def test_carried_facts(seed):
    """Carried: a packet has at most one dropped record and every served record precedes it (so a
    lane per record can tell its packet's last served record from its successor alone), and delay
    == the sum over S(p) of wait + service: the chain telescopes."""
    c = OC.random_case(seed)
    rc, res = OC.queue_ref(c, True, True)
    assert rc == QR.OK
    rc, _, delay, arrive, where = OC.ref(c, True, True, res)
    assert rc == QR.OK
    served, dropped, absent = DR.states(res)
    link = np.repeat(np.arange(len(c["cost_ps"])), np.diff(c["link_off"].astype(np.int64)))
    for p in range(c["n_packets"]):
        r = np.flatnonzero(c["packet"] == p)
        r = r[np.argsort(c["enter"][r], kind="stable")]
        assert dropped[r].sum() <= 1
        k = int(served[r].sum())
        assert served[r[:k]].all() and absent[r[k + 1:]].all() and (k == len(r) or dropped[r[k]])
        s = [QR.service(int(c["weight"][p]), int(c["cost_ps"][link[i]])) for i in r[:k]]
        assert int(delay[p]) == sum(int(res.wait[i]) + x for i, x in zip(r[:k], s))
        assert (int(where[p]) == (OR.NOTHING if not len(r) else OR.ARRIVED if k == len(r) else int(r[k])))
        assert int(arrive[p]) == (int(c["base"][p]) + int(delay[p]) if k == len(r) else MAX)


def test_first_order_rule():
    """First order a served crossing after a drop does not count, one at the drop's own time
    neither, and of two drops the earlier (then the smaller index) is the packet's."""
    M = MAX
    off = np.uint64([0, 3, 6])
    enter = np.uint64([10, 30, 50, 20, 30, 40])
    packet = np.uint32([0, 0, 0, 0, 0, 0])
    #       served   dropped  served    served   dropped  dropped
    wait = np.uint64([2, M, 0, 3, M, M])
    done = np.uint64([15, 30, 55, 25, 30, 40])
    rc, _, d, a, w = OR.outcomes(off, enter, packet, wait, done, 1, False, np.uint64([1000]))
    assert (rc, w.tolist(), d.tolist(), a.tolist()) == (QR.OK, [1], [5 + 5], [M])
    wait[[1, 4]] = 0  # only record 5 is dropped: everything before 40 counts
    done[[1, 4]] = [31, 37]
    rc, _, d, a, w = OR.outcomes(off, enter, packet, wait, done, 1, False, np.uint64([1000]))
    assert (rc, w.tolist(), d.tolist()) == (QR.OK, [5], [5 + 1 + 5 + 7])
    c = OC.ties()
    rc, _, d, a, w = OC.ref(c, False, True)
    r = [int(np.flatnonzero((c["packet"] == p) & (c["enter"] == t))[0]) for p, t in ((0, 100), (1, 200))]
    assert rc == QR.OK and d.tolist() == [10, 10] and w.tolist() == [r[0] + 1, r[1]] and a.tolist() == [M, M]
    assert c["packet"][r[0] + 1] == 0 and c["packet"][r[1]] == 1 and c["link_off"][1] == r[0] + 1
    # on a real first-order result: some packet has a served record behind its drop
    c = OC.long_chains(True)
    rc, res = OC.queue_ref(c, False, True)
    rc, _, d, a, w = OC.ref(c, False, True, res)
    r0 = np.flatnonzero(c["packet"] == 0)
    served, dropped, _ = DR.states(res)
    assert dropped[r0].sum() == 1 and served[r0].sum() == 2048 and int(w[0]) == int(r0[dropped[r0]][0])
    assert int(d[0]) == 0 and int(a[0]) == M
    rc, _, d, a, w = OC.ref(c, True, True)
    assert int(w[0]) == int(r0[0]) and int(d[0]) == 0 and int(a[0]) == M


@pytest.mark.parametrize("mode", OC.MODES, ids=OC.MODE_IDS)
def test_packets_without_a_record(mode):
    c0 = OC.random_case(3)
    c, empty = OC.with_empty(c0)
    base = c["base"].copy()
    base[empty[1]] = MAX  # (legal: nothing is added to it)
    c = dict(c, base=base)
    rc0, _, d0, a0, w0 = OC.ref(c0, *mode)
    rc, _, d, a, w = OC.ref(c, *mode)
    assert rc0 == rc == QR.OK
    keep = np.setdiff1d(np.arange(c["n_packets"]), empty)
    assert np.array_equal(d[keep], d0) and np.array_equal(a[keep], a0)
    for p in empty:
        assert (int(w[p]), int(d[p]), int(a[p])) == (OR.NOTHING, 0, int(base[p]))
    # (where is a record index: it moves with nothing here, the records are the same)
    assert np.array_equal(w[keep], w0)


@pytest.mark.parametrize("mode", OC.MODES, ids=OC.MODE_IDS)
def test_errors_and_overflow(mode):
    c = OC.random_case(5)
    pk = c["packet"].copy()
    pk[[7, 3]] = c["n_packets"]
    assert OC.ref(dict(c, packet=pk), *mode, OC.queue_ref(c, *mode)[1])[:2] == (QR.INVALID_ARG, 3)
    legal, p = OC.edge_base(c, *mode, 1)
    rc, _, d, a, w = OC.ref(legal, *mode)
    assert rc == QR.OK and int(a[p]) == MAX - 1 and int(w[p]) == OR.ARRIVED
    over, p2 = OC.edge_base(c, *mode, 0)
    rc, recs = OC.ref(over, *mode)[:2]
    assert p2 == p and rc == QR.TIME_OVERFLOW and recs == set(np.flatnonzero(c["packet"] == p).tolist())
    # a dropped packet never overflows, whatever its base
    rc, _, d, a, w = OC.ref(c, *mode)
    if (w < OR.ARRIVED).any():
        base = c["base"].copy()
        base[w < OR.ARRIVED] = MAX
        assert OC.ref(dict(c, base=base), *mode)[0] == QR.OK
    assert OR.check_args(5, None, 1, 1, 1) == OR.check_args(5, 1, 1, None, 1) == QR.INVALID_ARG
    assert OR.check_args((1 << 32) - 1, 1, 1, 1, 1) == OR.CAPACITY and OR.check_args((1 << 32) - 2, 1, 1, 1, 1) == QR.OK


def test_case_sizes():
    """The GPU cases have the record and packet counts they are named for, and every state."""
    for n in OC.RECORDS:
        assert len(OC.by_records(n)["enter"]) == n
    for P in OC.PACKETS:
        assert OC.by_packets(P)["n_packets"] == P
    for c, some, every in ((OC.all_dropped(), True, True), (OC.none_dropped(), False, False), (OC.last_hop_drop(), True, False)):
        rc, _, d, a, w = OC.ref(c, True, True)
        lost = w < OR.ARRIVED
        assert rc == QR.OK and bool(lost.any()) == some and bool(lost.all()) == every
    c = OC.last_hop_drop()
    rc, _, d, a, w = OC.ref(c, True, True)
    assert w.tolist() == [int(np.flatnonzero((c["packet"] == 0) & (c["enter"] == 140))[0]), OR.ARRIVED,
                          int(np.flatnonzero(c["packet"] == 2)[0])]
    assert d.tolist() == [20, 15, 0]  # (packet 0: 10 ns of service on link 0, 10 on link 1)
    for cut in (False, True):
        c = OC.long_chains(cut)
        n = np.bincount(c["packet"], minlength=c["n_packets"])
        assert n[0] == 2049 and n[1] == 65 and n[2:].max() <= 3


@pytest.mark.parametrize("name", ["tie", "k04", "k30"])
def test_real_traces_against_the_host_fold(oracle, name):
    """A fully watched trace: the carried outcome of every packet that arrived is the carried exit
    of its last record, as the host-side fold over the record arrays gives it."""
    from shadow_amd.link_queue import LinkQueueCarriedDropped, _exit_carried

    r = OC.real_trace(oracle, name)
    c, res, tr = r["case"], r["res"], r["tr"]
    rc, _, delay, arrive, where = OC.ref(c, True, True, res)
    assert rc == QR.OK
    served, dropped, absent = DR.states(res)
    queue = LinkQueueCarriedDropped(res.wait, res.done, res.ahead, res.link_free, res.busy, res.wait_max, res.wait_sum,
                                    res.ahead_max, dropped, res.drops, res.refused, absent, r["cur"], 0)
    exit_ns = _exit_carried(tr[4].copy(), tr[3], queue)
    last = np.full(c["n_packets"], -1, np.int64)
    order = np.argsort(tr[3], kind="stable")
    last[tr[1][order].astype(np.int64)] = order
    ok = where == OR.ARRIVED
    assert np.array_equal(arrive[ok], exit_ns[last[ok]])
    lost = where < OR.ARRIVED
    assert (exit_ns[last[lost]] == np.uint64(MAX)).all() and (arrive[lost] == np.uint64(MAX)).all()
    assert np.array_equal(lost, np.bincount(tr[1][dropped], minlength=c["n_packets"]) > 0)
    assert lost.any(), "no packet is lost"
    assert (ok & (delay > 0) & (arrive > c["base"])).any(), "no packet arrived late"
    assert (where == OR.NOTHING).any(), "no packet is without a record"


def test_flag_through_the_layers():
    from shadow_amd import _capi

    flag = OR.PACKETS_FLAG
    assert getattr(_capi, flag) == OR.PACKETS == 16
    with open(_capi.HEADER_PATH) as f:
        assert re.search(rf"^#define {flag} 0x10u$", f.read(), flags=re.M)
    with open(os.path.join(ROOT, "bindings", "shadow-gpu-sys", "src", "lib.rs")) as f:
        assert re.search(rf"^pub const {flag}: u32 = 16;$", f.read(), flags=re.M)


def test_python_surface():
    import shadow_amd
    from shadow_amd.graph import WHERE_ARRIVED, WHERE_NOTHING

    assert shadow_amd.PacketOutcomes._fields == ("delay_ns", "arrive_ns", "where", "lost", "drop_link", "arrive_dev")
    assert (WHERE_ARRIVED, WHERE_NOTHING) == (OR.ARRIVED, OR.NOTHING)
    for f in (shadow_amd.link_queue, shadow_amd.PathTree.link_queue_round, shadow_amd.Group.link_queue_round):
        p = inspect.signature(f).parameters["outcomes"]
        assert p.default is None and p.kind == p.KEYWORD_ONLY
    p = inspect.signature(shadow_amd.NetworkGraph.link_queue_device).parameters["outcomes"]
    assert p.default is False and p.kind == p.KEYWORD_ONLY
    p = inspect.signature(shadow_amd.PacketWire.push).parameters["deliver_time_ns"]
    assert p.default is None
