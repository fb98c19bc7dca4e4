"""The finite-buffer link-queue reference (tests/queue_drop_ref.py): a hand-written example with
every number written out, the event-driven simulation against the fixed-point loop under drops,
the identity at unlimited buffers, the two properties the library's kernels rest on (the limited
`done` never exceeds the unlimited one; restarting from an idle server at the unlimited queue's
busy-period heads changes nothing), the error rules, the conditions the GPU cases' inputs must meet
(test_queue_drop_gpu.py), and the flag through the layers.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import queue_carry_cases as CC
import queue_carry_ref as CR
import queue_cases as QC
import queue_drop_cases as DC
import queue_drop_ref as DR
import queue_ref as QR
from test_queue_carry_ref_cpu import _real

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX = DR.MAX


def _same(a, b, fields=DR.FIELDS):
    for k in fields:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype == DR.DTYPES[k] and np.array_equal(x, y), k


def _both(c):
    """The two carried statements agree; (Result, carried enter, iterations)."""
    rc, pair, want, cur, _ = DC.ref_carried(c)
    rj, pj, got, cj, iters = DC.ref_carried(c, jacobi=True)
    assert rc == rj == DR.OK and pair is None and pj is None
    _same(got, want)
    assert np.array_equal(cur, cj)
    return want, cur, iters


def test_hand_example():
    c, want, enter, first = DC.hand()
    got, cur, iters = _both(c)
    _same(got, want)
    assert np.array_equal(cur, enter) and iters == 2
    served, dropped, absent = DR.states(got)
    assert served.tolist() == [True, False, False, True, True, False]
    assert dropped.tolist() == [False, True, False, False, False, True]
    assert absent.tolist() == [False, False, True, False, False, False]
    # the carried enter time from the outputs alone: done - s - wait served, done dropped, 2^64 - 1 absent
    back = got.done.copy()
    back[served] = got.done[served] - np.uint64(10) - got.wait[served]
    assert np.array_equal(back, enter)
    # a packet dropped on link 0 is absent on link 1, where C is then served without the wait the
    # unlimited result gives it
    rc, _, unl, _, _ = CC.ref(c)
    assert rc == CR.OK and int(unl.wait[3]) == 9 and int(got.wait[3]) == 0
    # D is dropped on link 2 behind the carried B; the first-order flagged result serves it
    rc, _, fo = DC.ref(c)
    assert rc == DR.OK
    _same(fo, first)
    assert dropped[5] and int(fo.wait[5]) == 0


@pytest.mark.parametrize("seed", range(36))
def test_event_against_jacobi(seed):
    rng = np.random.default_rng(2000 + seed)
    c = CC.random_chains(seed, n_links=int(rng.integers(1, 9)), n_packets=int(rng.integers(1, 120)),
                         hops=(1, int(rng.integers(1, 7))), free_max=(0, 300)[seed % 2])
    c = DC.draw_limits(c, 3000 + seed)
    want, cur, iters = _both(c)
    assert iters >= 1
    if seed % 3 == 0:  # unit weights
        _both(dict(c, weight=None))


def test_the_random_instances_drop_and_lose():
    """Over the instances above: records dropped, records absent, records waiting."""
    drops = absent = waits = 0
    for seed in range(36):
        rng = np.random.default_rng(2000 + seed)
        c = CC.random_chains(seed, n_links=int(rng.integers(1, 9)), n_packets=int(rng.integers(1, 120)),
                             hops=(1, int(rng.integers(1, 7))), free_max=(0, 300)[seed % 2])
        res = DC.ref_carried(DC.draw_limits(c, 3000 + seed))[2]
        s, d, a = DR.states(res)
        drops, absent, waits = drops + int(d.sum()), absent + int(a.sum()), waits + int((res.wait[s] > 0).sum())
    assert drops > 100 and absent > 100 and waits > 100, (drops, absent, waits)


@pytest.mark.parametrize("seed", range(6))
def test_identity_at_unlimited_buffers(seed):
    c = CC.random_chains(40 + seed, n_links=5, n_packets=80, hops=(1, 4), free_max=(0, 200)[seed % 2])
    c = DC.with_limits(c, MAX)
    nl = len(c["cost_ps"])
    zero32, zero64 = np.zeros(nl, np.uint32), np.zeros(nl, np.uint64)
    rc, _, fo = DC.ref(c)
    rq, _, want = QC.ref(c)
    assert rc == rq == QR.OK
    for k in QR.FIELDS:
        assert np.array_equal(getattr(fo, k), getattr(want, k)), k
    assert np.array_equal(fo.drops, zero32) and np.array_equal(fo.refused, zero64)
    got, cur, iters = _both(c)
    rc, _, ev, cur2, _ = CC.ref(c)
    rc2, _, _, _, it2 = CC.ref(c, jacobi=True)
    assert rc == rc2 == CR.OK and np.array_equal(cur, cur2) and iters == it2
    for k in QR.FIELDS:
        assert np.array_equal(getattr(got, k), getattr(ev, k)), k
    assert np.array_equal(got.drops, zero32) and np.array_equal(got.refused, zero64)


def test_limit_zero():
    """A record is dropped whenever it would wait at all: every served record has wait 0."""
    c = DC.with_limits(QC.random_trace([0, 70, 300, 1], 5, free_max=100), 0)
    rc, _, res = DC.ref(c)
    served, dropped, _ = DR.states(res)
    assert rc == DR.OK and dropped.sum() > 50 and served.sum() > 50 and not res.wait[served].any()
    assert not res.wait_max.any() and not res.wait_sum.any()
    cc = DC.with_limits(CC.random_chains(9, n_links=4, n_packets=100), 0)
    got, _, _ = _both(cc)
    served, dropped, absent = DR.states(got)
    assert dropped.any() and absent.any() and not got.wait[served].any()


def test_fast_reference():
    """queue_drop_cases.fast (the large cases' reference) against the plain loop."""
    for seed, lim in ((1, 60), (2, 0), (3, 1), (4, MAX)):
        c = DC.periods([[3, 70, 1, 1, 200], [], [40]], seed, lim, free=50)
        rc, _, want = DC.ref(c)
        assert rc == DR.OK
        _same(DC.fast(c), want)
    c = DC.draw_limits(QC.random_trace([5, 0, 300, 64], 8, free_max=80), 9)
    _same(DC.fast(c), DC.ref(c)[2])


def _properties(c):
    """On a first-order case: the limited `done` is never above the unlimited one, and a restart
    from an idle server at every unlimited head gives the limited result."""
    n = len(c["enter"])
    lim_trace, unl_trace = [], []
    rc, _, res = DC.ref(c, trace=lim_trace)
    rq, _, _ = DC.ref(DC.with_limits(c, MAX), trace=unl_trace)
    assert rc == rq == DR.OK or (rc, rq) == (DR.OK, DR.TIME_OVERFLOW)
    assert len(lim_trace) == len(unl_trace) == n and all(a <= b for a, b in zip(lim_trace, unl_trace))
    # the unlimited heads: a segment's first record, or enter >= the unlimited done before it
    off = c["link_off"].astype(np.int64)
    first = set(off[:-1][off[1:] > off[:-1]].tolist())
    ent = c["enter"].tolist()
    heads = [i for i in range(n) if i in first or ent[i] >= unl_trace[i - 1]]
    # every period on its own: a link of one period, its server idle (free_in 0) unless it starts a segment
    link = np.repeat(np.arange(len(off) - 1), np.diff(off))
    wait, done = res.wait.copy(), res.done.copy()
    for a, b in zip(heads, heads[1:] + [n]):
        lk = int(link[a])
        assert b <= off[lk + 1]
        free = 0 if a not in first or c["free_in"] is None else int(c["free_in"][lk])
        w = None if c["weight"] is None else c["weight"]
        sub = dict(link_off=np.uint64([0, b - a]), enter=c["enter"][a:b], packet=None if w is None else c["packet"][a:b],
                   weight=w, cost_ps=c["cost_ps"][lk:lk + 1], free_in=np.uint64([free]), limit_ns=c["limit_ns"][lk:lk + 1])
        r = DC.ref(sub)[2]
        assert np.array_equal(r.wait, wait[a:b]) and np.array_equal(r.done, done[a:b]), (a, b)
    return len(heads), res


@pytest.mark.parametrize("seed", range(8))
def test_busy_period_properties(seed):
    c = QC.random_trace([0, 70, 300, 1, 129], 50 + seed, free_max=(0, 100)[seed % 2])
    c = DC.draw_limits(c, 60 + seed, limits=(0, 5, 20, 60))
    n_heads, res = _properties(c)
    assert 4 < n_heads < len(c["enter"]) and DR.states(res)[1].any()
    # an unsorted segment: the recurrence is a function of the arrays as given
    rng = np.random.default_rng(70 + seed)
    perm = np.concatenate([rng.permutation(np.arange(a, b)) for a, b in zip(c["link_off"][:-1].astype(np.int64),
                                                                            c["link_off"][1:].astype(np.int64))])
    _properties(dict(c, enter=c["enter"][perm], packet=c["packet"][perm]))


def test_properties_when_the_unlimited_scan_saturates():
    """The unlimited queue runs into 2^64 - 1 (free_in near it), which only merges periods; the
    limited one drops everything behind that server and stays clean."""
    c = DC.with_limits(QC.case([0, 6], [100, 110, 120, 130, 140, 150], cost_ps=[10**4], free_in=[MAX - 25]), 50)
    n_heads, res = _properties(c)
    assert n_heads == 1 and DR.states(res)[1].all() and res.link_free.tolist() == [MAX - 25]
    assert DC.ref(DC.with_limits(c, MAX))[0] == DR.TIME_OVERFLOW


def test_period_cases_have_their_periods():
    """queue_drop_cases.periods gives exactly the unlimited busy periods asked for, and a limit of
    60 drops, serves with a wait and serves without."""
    segs = [[1, 2, 31, 32, 33, 64, 65], [], [300, 1, 1, 5]]
    for touch in (False, True):
        c = DC.periods(segs, 11, 60, touch=touch)
        want = np.zeros(len(c["enter"]), bool)
        at = 0
        for p in [k for s in segs for k in s]:
            want[at] = True
            at += p
        assert np.array_equal(DC.period_heads(c), want)
    res = DC.ref(c)[2]
    served, dropped, _ = DR.states(res)
    assert dropped.sum() > 100 and (res.wait[served] > 0).sum() > 100 and (res.wait[served] == 0).sum() >= 10
    # a first record dropped by free_in
    c = DC.with_limits(DC.periods([[5]], 12, 60), 60)
    res = DC.ref(dict(c, free_in=np.uint64([1061])))[2]
    assert DR.states(res)[1][0] and int(res.ahead[0]) == 0


def test_errors():
    c, _, _, _ = DC.hand()
    bad_off = dict(c, link_off=np.uint64([0, 3, 2, 6]))
    assert DC.ref(bad_off)[:2] == (DR.INVALID_ARG, (1, DR.UMAX))
    assert DC.ref_carried(bad_off)[:2] == (DR.INVALID_ARG, (1, DR.UMAX))
    pk = c["packet"].copy()
    pk[[3, 4]] = 4, 7
    assert DC.ref(dict(c, packet=pk))[:2] == (DR.INVALID_ARG, (1, 1))
    assert DC.ref_carried(dict(c, packet=pk))[:2] == (DR.INVALID_ARG, (1, 1))
    # a served done reaching 2^64 - 1; behind a bad packet
    far = dict(c, free_in=np.uint64([0, 0, MAX - 12]), limit_ns=np.uint64([5, 5, MAX]))
    assert DC.ref(far)[:2] == (DR.TIME_OVERFLOW, (2, 1))
    assert DC.ref(dict(far, packet=pk))[:2] == (DR.INVALID_ARG, (1, 1))
    for f in (False, True):
        assert DC.ref_carried(far, jacobi=f)[:2] == (DR.TIME_OVERFLOW, None)
    # the same record dropped (the buffer holds 5 ns): it would have overflowed and does not
    near = dict(far, limit_ns=np.uint64([5, 5, 5]))
    rc, _, res = DC.ref(near)
    assert rc == DR.OK and DR.states(res)[1][4:].all() and res.link_free.tolist()[2] == MAX - 12
    for f in (False, True):
        rc, _, res = DC.ref_carried(near, jacobi=f)[:3]
        assert rc == DR.OK and DR.states(res)[1][4:].all()
    # done + gap reaching 2^64 - 1 with every done below it; one ns earlier is none; dropped on
    # link 0, the packet carries nothing
    for f in (False, True):
        o = DC.with_limits(CC.carry_overflow(0), MAX)
        assert DC.ref_carried(o, jacobi=f)[:2] == (DR.TIME_OVERFLOW, None)
        rc, _, res, cur = DC.ref_carried(DC.with_limits(CC.carry_overflow(1), MAX), jacobi=f)[:4]
        assert rc == DR.OK and res.done.tolist() == [MAX - 6, MAX - 1]
        rc, _, res, cur = DC.ref_carried(DC.with_limits(CC.carry_overflow(0), 5), jacobi=f)[:4]
        assert rc == DR.OK and res.wait.tolist() == [MAX, MAX] and res.done.tolist() == [100, MAX]
        assert res.drops.tolist() == [1, 0] and cur.tolist() == [100, MAX]
    # the iteration cap
    s = DC.with_limits(CC.staircase(6), MAX)
    assert DC.ref_carried(s, jacobi=True, cap=2)[:2] == (DR.CAPACITY, (2, DR.UMAX))


# ---- the real traces
def _limited(c, carried):
    """The case under the median rule, and the unlimited result of the same mode."""
    if carried:
        rc, _, unl, _, _ = CC.ref(c)
    else:
        rc, _, unl = QC.ref(c)
    assert rc == QR.OK
    return DC.with_limits(c, DR.median_limits(c["link_off"], unl.wait)), unl


@pytest.mark.parametrize("name", [None, "k04", "k30"], ids=lambda n: n or "tie")
def test_real_trace_conditions(oracle, name):
    c = _real(oracle, name)
    # first order
    lc, unl = _limited(c, False)
    rc, _, res = DC.ref(lc) if name else (DR.OK, None, DC.fast(lc))
    served, dropped, _ = DR.states(res)
    print(f"{name or 'tie'} first order: {len(served)} records, {int(dropped.sum())} dropped, "
          f"{int((res.wait[served] > 0).sum())} waiting")
    assert rc == DR.OK and dropped.any() and (res.wait[served] > 0).any()
    # carried
    lc, unl = _limited(c, True)
    rc, _, res, cur, _ = DC.ref_carried(lc)
    assert rc == DR.OK
    served, dropped, absent = DR.states(res)
    less = served & (res.wait < unl.wait)
    print(f"{name or 'tie'} carried: {int(dropped.sum())} dropped, {int(absent.sum())} absent, "
          f"{int((res.wait[served] > 0).sum())} waiting, {int(less.sum())} waiting less")
    assert dropped.any(), "no record dropped"
    assert (res.wait[served] > 0).any(), "no served record waits"
    assert absent.any(), "no record absent"
    assert less.any(), "no served record waits less than in the unlimited result"
    if name:  # (the tie round's fixed point on the plain loop takes minutes)
        rj, _, got, cj, iters = DC.ref_carried(lc, jacobi=True)
        print(f"{name}: {iters} iterations")
        assert rj == DR.OK and np.array_equal(cur, cj)
        _same(got, res)


# ---- the layers
def test_flag_through_the_layers():
    from shadow_amd import _capi

    flag = DR.DROP_FLAG
    assert getattr(_capi, flag) == 8
    with open(_capi.HEADER_PATH) as f:
        assert re.search(rf"^#define {flag} 0x8u$", f.read(), flags=re.M)
    with open(os.path.join(ROOT, "bindings", "shadow-gpu-sys", "src", "lib.rs")) as f:
        assert re.search(rf"^pub const {flag}: u32 = 8;$", f.read(), flags=re.M)


def test_python_surface():
    import shadow_amd
    from shadow_amd import Group, NetworkGraph, PathTree

    for f in (shadow_amd.link_queue, NetworkGraph.link_queue_device, PathTree.link_queue_round, Group.link_queue_round):
        p = inspect.signature(f).parameters["limit_ns"]
        assert p.default is None and p.kind is p.KEYWORD_ONLY
    base = shadow_amd.LinkQueueResult._fields
    assert shadow_amd.LinkQueueDropped._fields == base + ("dropped", "link_drops", "link_refused_ns")
    assert shadow_amd.LinkQueueCarriedDropped._fields == shadow_amd.LinkQueueDropped._fields + ("absent", "enter_ns",
                                                                                                "iterations")


def test_queue_limit_ns():
    from shadow_amd import queue_limit_ns

    assert queue_limit_ns(1500, 8000) == 12000 and queue_limit_ns(1, 1) == 1 and queue_limit_ns(0, 8000) == 0
    assert queue_limit_ns(3, 333) == 1 and queue_limit_ns(3, 334) == 2
    assert queue_limit_ns(2**63, 2**40) == MAX and queue_limit_ns(2**54, 1024000) == MAX
    assert queue_limit_ns(2**54 - 1, 1024000) == (2**54 - 1) * 1024
    got = queue_limit_ns([1, 2**60, 2**63], [1, 8000, 8000])
    assert got.dtype == np.uint64 and got.tolist() == [1, 2**63, MAX]
    assert queue_limit_ns(65536, [80, 8000]).tolist() == [5243, 524288]
