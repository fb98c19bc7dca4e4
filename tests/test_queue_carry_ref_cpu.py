"""The carried link-queue reference (tests/queue_carry_ref.py): a hand-written example with every
number written out, the event-driven simulation against the fixed-point loop, the properties the
definition promises, the conditions the GPU cases' inputs must meet (test_queue_carry_gpu.py),
asserted here so that the cases qualify by the reference alone, and the flag through the layers.
No GPU."""
import os
import re

import numpy as np
import pytest

import link_cases as LC
import queue_carry_cases as CC
import queue_carry_ref as CR
import queue_cases as QC
import queue_ref as QR
import sweep_cases as WC
import trace_cases as XC
import trace_ref as XR
from test_queue_ref_cpu import _table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    for k in QR.FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype == QR.DTYPES[k] and np.array_equal(x, y), k


def _both(c):
    """The two statements agree; (Result, carried enter, iterations)."""
    rc, pair, want, cur, _ = CC.ref(c)
    rj, pj, got, cj, iters = CC.ref(c, jacobi=True)
    assert rc == rj == CR.OK and pair is None and pj is None
    _same(got, want)
    assert np.array_equal(cur, cj)
    return want, cur, iters


def test_hand_example():
    c, want, enter, first = CC.hand()
    got, cur, iters = _both(c)
    _same(got, want)
    assert np.array_equal(cur, enter) and iters == 2
    # carried enter = done - s - wait
    assert np.array_equal(got.done - 10 - got.wait, enter)
    # the first-order result serves A ahead of C on link 1
    rc, _, fo = CC.first_order(c)
    assert rc == QR.OK
    _same(fo, first)
    assert fo.done[2] < fo.done[3] and got.done[2] > got.done[3]


@pytest.mark.parametrize("seed", range(30))
def test_event_against_jacobi(seed):
    rng = np.random.default_rng(1000 + seed)
    c = CC.random_chains(seed, n_links=int(rng.integers(1, 9)), n_packets=int(rng.integers(1, 120)),
                         hops=(1, int(rng.integers(1, 7))), free_max=(0, 300)[seed % 2])
    want, cur, iters = _both(c)
    assert iters >= 1
    if seed % 3 == 0:  # unit weights
        _both(dict(c, weight=None))


def test_generated_gpu_cases():
    """The segment lengths, the long chains and the hot link: both statements agree, times move
    and orders change."""
    c = CC.from_lengths([0, 1, 64, 65, 300, 0], 3, free_max=500)
    want, cur, iters = _both(c)
    assert all(CC.conditions(c, cur, iters)), CC.conditions(c, cur, iters)
    # (the larger ones through the event simulation alone: the loop takes an iteration per hop of
    # the longest chain, and its `ahead` count is quadratic)
    c = CC.long_chains()
    cnt = np.bincount(c["packet"])
    assert cnt[0] == CC.PIECE + 1 and cnt[1] == 65 and cnt[2:].max() <= 3
    rc, _, want, cur, _ = CC.ref(c)
    assert rc == CR.OK and want.wait.any() and CC.conditions(c, cur, 3) == (True, True, True)
    c = CC.hot_link()
    rc, _, want, cur, _ = CC.ref(c)
    assert rc == CR.OK and len(c["enter"]) == 10000 and int(np.diff(c["link_off"].astype(np.int64))[0]) == 5000
    assert CC.conditions(c, cur, 3) == (True, True, True)
    seg = slice(0, 5000)
    assert (np.argsort(cur[seg], kind="stable") != np.argsort(c["enter"][seg], kind="stable")).sum() > 1000
    c = CC.from_lengths(CC.SEGMENTS, 4, free_max=500)
    rc, _, want, cur, _ = CC.ref(c)
    assert rc == CR.OK and want.wait.any() and CC.conditions(c, cur, 3)[:2] == (True, True)
    assert set(np.bincount(c["packet"]).tolist()) == {1, 2, 3}


def test_cost_zero_gives_the_input_back():
    c = CC.random_chains(5, n_links=5, n_packets=80, costs=(0,))
    want, cur, iters = _both(c)
    assert np.array_equal(cur, c["enter"]) and not want.wait.any() and np.array_equal(want.done, c["enter"]) and iters == 1


def test_single_record_chains_equal_first_order():
    c = CC.single_records([0, 70, 300, 1], 31)
    assert len(set(c["packet"].tolist())) == len(c["packet"])
    want, cur, iters = _both(c)
    rc, _, fo = QC.ref(c)
    assert rc == QR.OK and iters == 1 and np.array_equal(cur, c["enter"])
    _same(want, fo)


def test_permuting_a_links_records_permutes_the_outputs():
    c = CC.random_chains(7, n_links=5, n_packets=100, hops=(1, 4))
    want, cur, _ = _both(c)
    s, perm = CC.shuffled(c, 8)
    assert not np.array_equal(perm, np.arange(len(perm)))
    got, cur2, _ = _both(s)
    for k in QR.RECORD_FIELDS:
        assert np.array_equal(getattr(got, k), getattr(want, k)[perm]), k
    for k in QR.FIELDS[3:]:
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    assert np.array_equal(cur2, cur[perm])


@pytest.mark.parametrize("k", CC.STAIRS)
def test_staircase(k):
    c = CC.staircase(k)
    want, cur, iters = _both(c)
    assert iters >= k
    # every packet reaches its second link 24 ns after it entered its first: 9 waiting, 10 served, 5 on the way
    second = np.array([int(cur[(c["packet"] == j) & (c["enter"] == 6 + 25 * j)][0]) for j in range(k)])
    assert second.tolist() == [25 + 25 * j for j in range(k)]
    assert CR.jacobi(c["link_off"], c["enter"], c["packet"], c["weight"], n_packets=k + 1, cost_ps=c["cost_ps"],
                     cap=k - 1)[:2] == (CR.CAPACITY, (k - 1, CR.UMAX))


def test_errors():
    c, _, _, _ = CC.hand()
    assert CC.ref(dict(c, link_off=np.uint64([0, 3, 2, 6])))[:2] == (CR.INVALID_ARG, (1, CR.UMAX))
    pk = c["packet"].copy()
    pk[[3, 4]] = 3, 7
    assert CC.ref(dict(c, packet=pk))[:2] == (CR.INVALID_ARG, (1, 1))
    assert CC.ref(dict(c, packet=pk, weight=None, n_packets=8))[0] == CR.OK
    # packet 2's records (3 and 4) at one time: the smaller record, on its link; behind a bad packet
    twin = dict(c, enter=np.uint64([100, 101, 106, 100, 100, 107]))
    for f in (False, True):
        assert CC.ref(twin, jacobi=f)[:2] == (CR.INVALID_ARG, (1, 1))
        assert CC.ref(dict(twin, packet=np.uint32([1, 0, 0, 2, 2, 9])), jacobi=f)[:2] == (CR.INVALID_ARG, (2, 1))
        far = dict(c, free_in=np.uint64([0, CR.MAX - 12, 0]))
        assert CC.ref(far, jacobi=f)[:2] == (CR.TIME_OVERFLOW, None)
        # done + gap reaching 2^64 - 1 with every done below it; one ns earlier is no error
        assert CC.ref(CC.carry_overflow(0), jacobi=f)[:2] == (CR.TIME_OVERFLOW, None)
        rc, _, res, cur = CC.ref(CC.carry_overflow(1), jacobi=f)[:4]
        assert rc == CR.OK and res.done.tolist() == [CR.MAX - 6, CR.MAX - 1] and int(cur[1]) == CR.MAX - 1


# ---- the real traces
def _real(oracle, name):
    """(case, payload) of the tie round (name None) or a sweep graph's round."""
    if name is None:
        g = LC.tie_graph()
        nodes, lat, pred = _table(oracle, g)
        hosts, pk, _ = XC.tie_round()
        tr = XR.trace(g, nodes, (0, g["n"]), pred, lat, hosts, pk)
        cost = np.full(XR.n_links(g), QC.TIE_COST, np.uint64)
    else:
        c, r = WC.case(name), WC.refs(oracle, name)[0]
        pk, status = QC.sweep_round(c)
        tr = XR.trace(c["g"], c["nodes"], (0, c["g"]["n"]), r["pred"], r["lat"], c["hosts"], pk, status)
        cost = QC.sweep_costs(name, XR.n_links(c["g"]))
    return CC.case(tr[0], tr[3], tr[1], pk["payload"], cost)


@pytest.mark.parametrize("name", [None] + list(CC.SWEEP_NAMES), ids=lambda n: n or "tie")
def test_real_trace_conditions(oracle, name):
    c = _real(oracle, name)
    rc, _, want, cur, iters = CC.ref(c, jacobi=True)
    assert rc == CR.OK
    moved, order, three = CC.conditions(c, cur, iters)
    print(f"{name or 'tie'}: {len(cur)} records, {int((cur != c['enter']).sum())} moved, order changes: {order}, "
          f"{iters} iterations")
    assert moved, "no record's carried enter differs from the input"
    assert order, "no link's service order differs from the input order"
    assert three, f"{iters} iterations"
    rc, _, ev, cur2, _ = CC.ref(c)
    assert rc == CR.OK and np.array_equal(cur, cur2)
    _same(want, ev)


# ---- the layers
def test_flag_through_the_layers():
    from shadow_amd import _capi

    flag = CC.CARRY_FLAG
    assert getattr(_capi, flag) == 4
    with open(_capi.HEADER_PATH) as f:
        assert re.search(rf"^#define {flag} 0x4u$", f.read(), flags=re.M)
    with open(os.path.join(ROOT, "bindings", "shadow-gpu-sys", "src", "lib.rs")) as f:
        assert re.search(rf"^pub const {flag}: u32 = 4;$", f.read(), flags=re.M)
    with open(os.path.join(ROOT, "shadow_amd", "csrc", "sg_knobs.h")) as f:
        assert re.search(r"^//\s+SG_LINK_QUEUE_CARRY_ITERS \| 4096 \| ", f.read(), flags=re.M)


def test_python_surface():
    import inspect

    import shadow_amd
    from shadow_amd import Group, PathTree

    assert shadow_amd.LinkQueueCarried._fields == shadow_amd.LinkQueueResult._fields + ("enter_ns", "iterations")
    for f in (shadow_amd.link_queue, PathTree.link_queue_round, Group.link_queue_round):
        p = inspect.signature(f).parameters["carry"]
        assert p.default is False and p.kind is p.KEYWORD_ONLY
