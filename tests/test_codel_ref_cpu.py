"""The CoDel model (codel_ref.py) and the boundary cases (codel_cases.py), checked on the CPU:
the model equals the oracle on every case, form and on the random streams; it passes the
reference's own unit tests (codel_queue.rs:332-534); the cases reach every arm and every side
of every comparison; and every single-site mutation of the model is caught by a named case."""
import numpy as np
import pytest

import codel_cases as cc
import codel_ref as ref

T0, MS = cc.T0, cc.MS
T, I, N = cc.T, cc.I, cc.N
MOCK_LEN = 20 + 8 + 1000   # PacketRc::new_ipv4_udp_mock: IPv4 + UDP headers + 1000 B payload
BATCHES = [(cap, form) for cap in (4, 64) for form in cc.FORMS]


def _batch(cap, form):
    cs = [c for c in cc.of_cap(cap) if cc.has_form(c, form)]
    return (cs,) + cc.build(cs, form, cap)


def _same(a, b, what=""):
    """Two states key by key; the ring at the live slots [head, tail) modulo 2^32."""
    for k in ref.SCALARS:
        assert np.array_equal(a[k], b[k]), (what, k)
    i = ref.live_slots(b)
    for k in ("ring_pkt", "ring_ts", "ring_len"):
        assert np.array_equal(a[k][i], b[k][i]), (what, k)


def _outcomes(cs, st, calls, res, status, base):
    """Per case: its pop results, its packets' statuses, its scalars and its live ring slots."""
    cap, out = st["cap"], []
    for i in range(len(cs)):
        n = (int(st["tail"][i]) - int(st["head"][i])) % ref.M32
        slots = [i * cap + (int(st["head"][i]) + j) % cap for j in range(min(n, cap))]
        out.append((tuple(tuple(r[c[0] == i].tolist()) for r, c in zip(res, calls)),
                    tuple(status[base[i]:base[i + 1]].tolist()), tuple(int(st[k][i]) for k in ref.SCALARS),
                    tuple((int(st["ring_pkt"][s]), int(st["ring_ts"][s]), int(st["ring_len"][s])) for s in slots)))
    return out


def _model(cs, st, calls, base, trace=None, variant=None):
    st, status = ref.copy_state(st), np.zeros(base[-1], np.uint8)
    res = [ref.run(st, *c, status, trace=trace, variant=variant) for c in calls]
    return _outcomes(cs, st, calls, res, status, base)


# ---- 1. the model equals the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("cap,form", BATCHES)
def test_model_equals_oracle_on_cases(oracle, cap, form):
    """Batched (two calls) and one call per event; the expected drop counts the cases carry."""
    cs, st0, calls, base = _batch(cap, form)
    sm, so, s1 = ref.copy_state(st0), ref.copy_state(st0), ref.copy_state(st0)
    km, ko, k1 = (np.zeros(base[-1], np.uint8) for _ in range(3))
    for c in calls:
        rm = ref.run(sm, *c, km)
        ro = oracle.codel_run(so, *c, ko)
        r1 = np.array([oracle.codel_run(s1, *(a[i:i + 1] for a in c), k1)[0] for i in range(len(c[0]))], np.uint32)
        assert np.array_equal(rm, ro) and np.array_equal(r1, ro)
    assert np.array_equal(km, ko) and np.array_equal(k1, ko)
    _same(sm, so, "model")
    _same(s1, so, "one event per call")
    for i, c in enumerate(cs):
        if "drops" in c["expect"]:
            assert int((km[base[i]:base[i + 1]] == ref.DROPPED).sum()) == c["expect"]["drops"], c["name"]


def _stream_of_cpu_test():
    """test_codel_cpu.py::test_batched_equals_one_at_a_time's stream."""
    rng = np.random.default_rng(5)
    H, E = 7, 3000
    host = np.sort(rng.integers(0, H, E)).astype(np.uint32)
    kind = (rng.random(E) < 0.45).astype(np.uint8)
    t = np.zeros(E, np.uint64)
    for h in range(H):
        idx = np.nonzero(host == h)[0]
        t[idx] = T0 + np.cumsum(rng.integers(0, 3 * MS, len(idx))).astype(np.uint64)
    return H, (host, kind, t, np.arange(E, dtype=np.uint32), rng.integers(40, 1500, E).astype(np.uint32))


def test_model_equals_oracle_on_random_streams(oracle):
    H, ev = _stream_of_cpu_test()
    streams = [(H, [ev])]
    for gap_ms, p_pop in ((3, 0.45), (1, 0.3), (20, 0.5)):   # test_codel_gpu._stream, small: three calls
        rng, t0, calls = np.random.default_rng(gap_ms), T0 + 10**9, []
        for c in range(3):
            calls.append(cc.stream(rng, 20, 3000, t0, gap_ms, p_pop, n_pkt0=c * 3000))
            t0 = int(calls[-1][2].max()) + 1
        streams.append((20, calls))
    for H, calls in streams:
        n = sum(len(c[0]) for c in calls)
        sm, so, km, ko = ref.new_state(H, 4096), oracle.codel_state(H, 4096), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        for c in calls:
            assert np.array_equal(ref.run(sm, *c, km), oracle.codel_run(so, *c, ko))
        assert np.array_equal(km, ko) and (ko == 2).any() and (ko == 1).any()
        _same(sm, so)


# ---- 2. the reference's unit tests through the model ---------------------------------------------
def mock_time_millis(ms):   # network/mod.rs:26-29
    return T0 + ms * MS


class OneQueue(ref.Queue):
    def __init__(self):
        super().__init__(64, {})
        self.next_pkt = 0

    def push_mock(self, now):
        self.push(self.next_pkt, MOCK_LEN, now)
        self.next_pkt += 1

    def __len__(self):
        return (self.tail - self.head) % ref.M32

    mode_drop = property(lambda s: bool(s.flags & ref.F_DROP))
    iend = property(lambda s: s.interval_end if s.flags & ref.F_IEND else None)
    dnext = property(lambda s: s.drop_next if s.flags & ref.F_DNEXT else None)


def test_reference_empty_and_push_pop():   # codel_queue.rs:332-363
    q, now = OneQueue(), mock_time_millis(1000)
    assert len(q) == 0 and q.pop(now) == ref.NONE
    for i in range(1, 11):
        assert len(q) == i - 1
        q.push_mock(now)
        assert len(q) == i
    for i in range(1, 11):
        assert len(q) == 10 - i + 1
        assert q.pop(now) != ref.NONE
        assert len(q) == 10 - i
    assert q.pop(now) == ref.NONE


def test_reference_control_law():   # codel_queue.rs:365-386
    q, now = OneQueue(), mock_time_millis(1000)
    for i in range(2):
        assert q.apply_control_law(now, i) - now == I
    for i in range(2, 20):
        # f64::round of the same quotient, taken another way (no ties at these counts)
        assert q.apply_control_law(now, i) - now == int(np.floor(float(I) / np.sqrt(np.float64(i)) + 0.5))


def test_reference_interval():   # codel_queue.rs:388-431
    q, start = OneQueue(), mock_time_millis(1000)
    for _ in range(5):
        q.push_mock(start)
    assert q.bytes > ref.MTU and q.iend is None
    psd = lambda now, sd: q.process_standing_delay(now, sd, q.bytes)
    assert not psd(start + T - MS, T - MS) and q.iend is None
    assert not psd(start + T, T) and q.iend == start + T + I
    assert psd(start + T + I, T + I) and q.iend == start + T + I
    assert psd(start + T + 2 * I, T + 2 * I) and q.iend == start + T + I
    assert not psd(start + T + 2 * I, MS) and q.iend is None


def test_reference_mode():   # codel_queue.rs:433-483
    q, start = OneQueue(), mock_time_millis(1000)
    for _ in range(6):
        q.push_mock(start)
    assert q.bytes > ref.MTU and len(q) == 6 and not q.mode_drop
    for now, left in ((start + T - MS, 5), (start + T, 4), (start + T + I - MS, 3)):
        q.pop(now)
        assert len(q) == left and not q.mode_drop
    q.pop(start + T + I)
    assert len(q) == 1 and q.mode_drop
    for _ in range(3):
        q.push_mock(start + T + 2 * I - MS)
    q.pop(start + T + 2 * I)
    assert not q.mode_drop


def test_reference_drop_empty():   # codel_queue.rs:485-492
    q = OneQueue()
    q.flags |= ref.F_DROP
    q.pop(mock_time_millis(1000))
    assert not q.mode_drop


def test_reference_drop_many():   # codel_queue.rs:494-534
    q, start, end, n = OneQueue(), mock_time_millis(1000), mock_time_millis(1000000), 20
    for _ in range(n):
        q.push_mock(start)
    assert len(q) == n and not q.mode_drop
    q.pop(start + T)
    assert len(q) == n - 1 and q.cur == 0 and q.prev == 0 and not q.mode_drop
    assert not q.was_dropping_recently(start + T)
    q.pop(start + T + I)
    assert len(q) == n - 3 and q.cur == 1 and q.prev == 1 and q.dnext is not None and q.mode_drop
    assert q.was_dropping_recently(start + T + I) and q.should_drop(end)
    q.pop(end)
    assert len(q) == 1 and q.cur == n - 4 and not q.mode_drop


# ---- 3. coverage is a condition -------------------------------------------------------------------
def test_cases_reach_every_arm_and_every_side():
    trace = {}
    for cap, form in BATCHES:
        cs, st, calls, base = _batch(cap, form)
        if form == "ring":
            assert len(cs) == len(cc.of_cap(cap))   # no case left out
        _model(cs, st, calls, base, trace=trace)
    want = list(ref.ARMS) + [c + s for c in ref.COMPARISONS for s in (":lt", ":eq", ":gt")]
    want += ["drop_exit:" + w for w in ref.DROP_EXITS] + ["drops_per_pop:%d" % k for k in (0, 1, 2, 3, 5, 12)]
    assert [k for k in want if not trace.get(k)] == []
    assert [k for k in trace if k not in want and not k.startswith("drops_per_pop:")] == []   # ARMS is complete
    assert sum(len(cc.of_cap(cap)) for cap in (4, 64)) == len(cc.CASES)


def test_law_ties_are_the_listed_counts():
    """The counts whose quotient is an exact tie: where round (half away from zero), rint and a
    quotient one ulp off part.  Exact: q - floor(q) loses nothing below 2^52."""
    ties = [c for c in cc.LAW_COUNTS if (lambda q: q - np.floor(q) == 0.5)(float(I) / np.sqrt(np.float64(c)))]
    assert tuple(ties) == cc.LAW_TIES
    assert [ref.law_increment(c) for c in cc.LAW_TIES] == [195313, 39063, 7813, 1]
    assert [ref.law_increment(c, "law-rint") for c in cc.LAW_TIES] == [195312, 39062, 7812, 0]


# ---- 4. the cases have teeth ------------------------------------------------------------------------
def _gpu_streams(H, E):
    """test_codel_gpu.py::test_random_streams_over_calls (there: 500 hosts, 3 x 60k events)."""
    out = []
    for gap_ms, p_pop in ((3, 0.45), (1, 0.3), (20, 0.5)):
        rng, t0, calls = np.random.default_rng(gap_ms), T0 + 10**9, []
        for c in range(3):
            calls.append(cc.stream(rng, H, E, t0, gap_ms, p_pop, n_pkt0=c * E))
            t0 = int(calls[-1][2].max()) + 1
        out.append(calls)
    return out


def _stream_run(calls, variant, truth=None):
    """The end of every call (results, statuses, state); against truth: the first call that differs."""
    H, n = int(max(c[0].max() for c in calls)) + 1, sum(len(c[0]) for c in calls)
    st, status, ends = ref.new_state(H, 4096), np.zeros(n, np.uint8), []
    for i, c in enumerate(calls):
        try:
            res = ref.run(st, *c, status, variant=variant)
        except ValueError:
            return i
        end = (res, status.copy(), {k: st[k].copy() for k in ref.SCALARS})
        if truth is None:
            ends.append(end)
        elif not (np.array_equal(end[0], truth[i][0]) and np.array_equal(end[1], truth[i][1]) and all(
                np.array_equal(end[2][k], truth[i][2][k]) for k in ref.SCALARS)):
            return i
    return ends if truth is None else None


def _one(c, v):   # a mutation may overrun a ring: one case at a time
    st, calls, base = cc.build([c], "ring", c["cap"])
    try:
        return _model([c], st, calls, base, variant=v)[0]
    except ValueError:
        return None


def test_every_variant_is_killed_by_a_case():
    """Every single-site mutation of the model changes the pop results, the statuses or the end
    state of at least one case (ring form); the first such case is printed.  The two that none
    can catch are codel_ref.UNCATCHABLE, with the reason."""
    truth = [_one(c, None) for c in cc.CASES]
    alive = []
    print()
    for v in ref.VARIANTS:
        killers = [c["name"] for c, want in zip(cc.CASES, truth) if _one(c, v) != want]
        print("%-28s killed by %3d cases, first %s" % (v, len(killers), killers[0] if killers else "-"))
        if not killers:
            alive.append(v)
    assert alive == sorted(ref.UNCATCHABLE)


def stream_survivors(H, E, show=False):
    """The variants that test_random_streams_over_calls's streams (model against mutated model) do not notice."""
    streams = [(calls, _stream_run(calls, None)) for calls in _gpu_streams(H, E)]
    survive = []
    for v in ref.VARIANTS:
        by_stream = any(_stream_run(calls, v, truth) is not None for calls, truth in streams)
        if show:
            print("%-28s random streams: %s" % (v, "killed" if by_stream else "SURVIVES"))
        if not by_stream:
            survive.append(v)
    return survive


def test_which_variants_the_random_streams_miss():
    """What the boundary cases are measured against: random streams do not notice a comparison
    that holds <= for <, the rounding of the 2^18 tie, a delta that wraps or a ring counter not
    taken modulo 2^32.  Here a tenth of the GPU test's hosts at its ~120 events per host and call;
    `python tests/test_codel_ref_cpu.py` prints the table at the GPU test's own size (20 s)."""
    survive = set(stream_survivors(50, 6000))
    assert set(ref.UNCATCHABLE) <= survive
    assert {"sd<=T", "now>iend", "now>dnext", "recent<=16I", "delta-wraps", "law-rint", "counters-not-modular"} <= survive


def test_reciprocal_control_law_search():
    """codel_ref.UNCATCHABLE["law-rcp-mul"]: the searched counts, all agreeing."""
    def steps(c, rcp):
        s = np.sqrt(c.astype(np.float64))
        q = float(I) * (1.0 / s) if rcp else float(I) / s
        return np.floor(q) + (q - np.floor(q) >= 0.5)

    c = np.arange(1, 2**22 + 1, dtype=np.int64)
    assert np.array_equal(steps(c, False), steps(c, True))
    m = np.arange(2000, dtype=np.float64)
    near = (np.floor((float(I) / (m + 0.5))**2)[:, None] + np.arange(-50, 51)[None, :]).ravel()
    assert np.array_equal(steps(near, False), steps(near, True))
    assert all(ref.law_increment(k) == ref.law_increment(k, "law-rcp-mul") for k in cc.LAW_COUNTS)


# ---- 5. a few cases by hand -----------------------------------------------------------------------
def _by_hand(name, form="ring"):
    c = cc.BY_NAME[name]
    st, calls, base = cc.build([c], form, c["cap"])
    status = np.zeros(base[-1], np.uint8)
    res = [int(r) for call in calls for r, k in zip(ref.run(st, *call, status), call[1]) if k == ref.POP]
    return res, status.tolist(), {k: int(st[k][0]) for k in ref.SCALARS}


D, IE, DN = ref.F_DROP, ref.F_IEND, ref.F_DNEXT


@pytest.mark.parametrize("form", cc.FORMS)
def test_by_hand_the_2_18_tie(form):
    """law/count=262144/entry.  Store mode, interval_end = N due, cur = 2^18, prev = 0, drop_next =
    N - 1 set; four 1,000 B packets 50 ms old.  pop(N): packet 0 leaves 3,000 B > MTU, 50 ms >=
    TARGET, N >= interval_end: ok to drop, Store mode -> drop_from_store_mode.  Packet 0 dropped;
    packet 1 popped (2,000 B left, interval_end stays) and returned.  delta = 2^18 - 0, N is 1 ns
    past drop_next < 16 intervals, delta > 1: cur = 2^18.  sqrt(2^18) = 512, 1e8 / 512 = 195,312.5,
    a tie: away from zero 195,313.  drop_next = N + 195,313; prev = 2^18; Drop mode."""
    res, status, st = _by_hand("law/count=262144/entry", form)
    assert res == [1] and status == [2, 1, 0, 0]
    assert st == dict(flags=D | IE | DN, interval_end=N, drop_next=N + 195313, cur=2**18, prev=2**18, bytes=2000,
                      head=2, tail=4)


@pytest.mark.parametrize("form", cc.FORMS)
def test_by_hand_three_drops_in_one_pop(form):
    """drop/cur=1/k=3/on.  Drop mode, cur = prev = 1, drop_next = N, seven old 1,000 B packets,
    pop at N + 70,710,678 + 57,735,027 = N + 128,445,705.  Packet 0 is ok to drop (6,000 B left).
    Loop: now >= N: drop 0, cur 2, packet 1 ok, drop_next = N + round(1e8 / sqrt 2) = N + 70,710,678;
    now >= that: drop 1, cur 3, packet 2 ok, drop_next += round(1e8 / sqrt 3) = 57,735,027 -> N +
    128,445,705; now == that: drop 2, cur 4, packet 3 ok (3,000 B left), drop_next += 1e8 / 2 =
    50,000,000 -> N + 178,445,705 > now: packet 3 returned.  The second pop at the same time pops
    packet 4 (2,000 B left: still ok to drop) but drop_next is ahead: returned, no drop.  One ns
    earlier the third drop is not due."""
    res, status, st = _by_hand("drop/cur=1/k=3/on", form)
    assert res == [3, 4] and status == [2, 2, 2, 1, 1, 0, 0]
    assert st == dict(flags=D | IE | DN, interval_end=N - 10 * I, drop_next=N + 178445705, cur=4, prev=1, bytes=2000,
                      head=5, tail=7)
    res, status, st = _by_hand("drop/cur=1/k=3/before", form)
    assert res == [2, 3] and status == [2, 2, 1, 1, 0, 0, 0]
    assert (st["drop_next"], st["cur"], st["head"]) == (N + 128445705, 3, 4)


def test_by_hand_the_16_interval_edge():
    """entry/delta=2/dnext=16I-1, 16I, 16I+1.  Store mode, interval_end = N due, cur = 7, prev = 5,
    five old packets; pop(N) drops packet 0 and returns packet 1.  delta = 2 > 1, so all rests on
    was_dropping_recently: N - drop_next < 1,600,000,000.  1,599,999,999: cur = 2, drop_next = N +
    70,710,678.  1,600,000,000 and 1,600,000,001: cur = 1, drop_next = N + 100,000,000.  The second
    pop, at N + 1, is in Drop mode before drop_next: packet 2 returned."""
    for edge, cur, step in (("16I-1", 2, 70710678), ("16I", 1, 10**8), ("16I+1", 1, 10**8)):
        res, status, st = _by_hand("entry/delta=2/dnext=" + edge)
        assert res == [1, 2] and status == [2, 1, 1, 0, 0]
        assert st == dict(flags=D | IE | DN, interval_end=N, drop_next=N + step, cur=cur, prev=cur, bytes=2000, head=3,
                          tail=5)


def test_by_hand_the_mtu_edge():
    """mtu/left=1500|1501/popped=1.  Store mode, interval_end = N due; packets of 1, 750 and 750 or
    751 B, 50 ms old; pop(N) twice.  1,500 left: at most one MTU, good: packet 0 returned and
    interval_end cleared (the 1,501 B before the pop do not count); packet 1 leaves 750 B: good.
    1,501 left: bad and due: Store -> drop packet 0; packet 1 leaves 751 B: good, interval_end
    cleared, returned; no drop_next before: cur = 1, drop_next = N + 100,000,000, Drop mode.  The
    second pop takes packet 2 (0 B left): good, back to Store mode."""
    res, status, st = _by_hand("mtu/left=1500/popped=1")
    assert res == [0, 1] and status == [1, 1, 0]
    assert st == dict(flags=0, interval_end=N, drop_next=0, cur=0, prev=0, bytes=750, head=2, tail=3)
    res, status, st = _by_hand("mtu/left=1501/popped=1")
    assert res == [1, 2] and status == [2, 1, 1]
    assert st == dict(flags=DN, interval_end=N, drop_next=N + 10**8, cur=1, prev=1, bytes=0, head=3, tail=3)


def test_by_hand_the_entry_that_finds_the_queue_empty():
    """entry/queue-empty-after-drop.  One old packet, 6,000 B on the count (5,000 more than the
    ring holds), interval_end = N due.  pop(N): 5,000 B > MTU left: ok to drop; dropped; the second
    codel_pop finds no element: interval_end cleared, none returned -- by drop_from_store_mode,
    after it set Drop mode, so the mode stays (pop's own "queue empty" arm is not taken).
    cur = 1, drop_next = N + 1e8.  push at N + 1 (6,000 B), pop at N + 2: 5,000 B left but 1 ns
    old: good, returned, Store mode."""
    res, status, st = _by_hand("entry/queue-empty-after-drop")
    assert res == [ref.NONE, 1] and status == [2, 1]
    assert st == dict(flags=DN, interval_end=N, drop_next=N + 10**8, cur=1, prev=1, bytes=5000, head=2, tail=2)
    c = cc.BY_NAME["entry/queue-empty-after-drop"]
    st, calls, base = cc.build([c], "ring", 64)
    ref.run(st, *(a[:1] for a in calls[1]), np.zeros(2, np.uint8))
    assert st["flags"][0] == D | DN   # after the first pop alone: Drop mode, no interval


if __name__ == "__main__":
    stream_survivors(500, 60000, show=True)
