"""The link-queue reference (tests/queue_ref.py): a hand-written example with every output written
out, the numpy closed form against the plain loop, the error rules, the conditions the GPU cases'
inputs must meet (test_queue_gpu.py), asserted here so that the cases qualify by the reference
alone, and the new entry point through the layers.  No GPU.

The cap on the real traces -- some record with ahead >= 64, some link with a positive wait, some
link with an idle gap -- holds for trace_cases.tie_round() and wide_round() under one cost for
every link, and for the 40 sweep graphs under one cost per link drawn from {0, 80, 8,000, 10^6}
ps.  The sweep graphs take a round of queue_cases' own: the rounds of sweep_cases put at most 171
records on a link, and on 33 of the 40 graphs fewer than 65, where no cost gives ahead >= 64."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import group_trace_cases as GC
import link_cases as LC
import queue_cases as QC
import queue_ref as QR
import sweep_cases as WC
import trace_cases as XC
import trace_ref as XR
import tree_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX = QR.MAX


def _same(a, b):
    for k in QR.FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype == QR.DTYPES[k] and np.array_equal(x, y), k


def test_hand_example():
    c, want = QC.hand()
    rc, pair, got = QC.ref(c)
    assert rc == QR.OK and pair is None
    _same(got, want)
    _same(QC.ref(c, closed=True), want)
    # without free_in link 2 is idle between its records, link 0 unchanged (it was free by 5 < 10)
    rc, _, got = QC.ref(dict(c, free_in=None))
    assert rc == QR.OK and got.wait.tolist() == [0, 14, 0, 2, 0, 0] and got.link_free.tolist() == [37, 0, 60]
    assert got.ahead.tolist() == [0, 1, 0, 1, 0, 0]
    # unit weights: link 0's services are ceil(1.5) = 2 each
    rc, _, got = QC.ref(dict(c, packet=None, weight=None))
    assert rc == QR.OK and got.done.tolist() == [12, 14, 32, 34, 101, 102] and got.busy.tolist() == [8, 0, 2]


def test_service():
    assert [QR.service(w, c) for w, c in ((0, 999), (1, 1), (1, 999), (1, 1000), (1, 1001), (1500, 80), (1500, 8000))] == \
        [0, 1, 1, 1, 2, 120, 12000]
    assert QR.service(2**32 - 1, 1001) == 4299262263  # ceil(4294967295 * 1.001)
    assert QR.service(2**32 - 1, 2**64 - 1) == MAX and QR.service(1000, 2**64 - 1) == MAX
    assert QR.service(1000, 2**64 - 2) == MAX - 1 and QR.service(999, 2**64 - 1) == -(-999 * MAX // 1000)
    assert QR.service(5, 0) == 0


@pytest.mark.parametrize("seed", range(12))
def test_closed_form(seed):
    """Random small segments, empty links among them, free_in below, inside and above a segment's
    arrivals; the unit-weight form."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 50, int(rng.integers(1, 40)))
    c = QC.random_trace(lengths, seed, free_max=(0, 100, 3000)[seed % 3], weighted=seed % 4 != 3)
    rc, pair, want = QC.ref(c)
    assert rc == QR.OK
    _same(QC.ref(c, closed=True), want)
    if len(want.wait) > 200 and c["weight"] is not None:
        assert want.wait.any() and (want.wait == 0).any() and want.ahead.max() > 1


def test_closed_form_on_the_gpu_cases():
    """The packed lengths and the tile edges: the loop and the closed form agree, queues build
    and drain."""
    for lengths, seed in ((QC.packed_lengths(), 5), (QC.tile_edge_lengths(), 6)):
        c = QC.random_trace(lengths, seed, free_max=100)
        rc, _, want = QC.ref(c)
        assert rc == QR.OK and want.ahead.max() >= 64 and (want.wait == 0).sum() > 100
        _same(QC.ref(c, closed=True), want)


def test_errors():
    c, _ = QC.hand()
    for off, link in (([1, 4, 4, 6], 0), ([0, 4, 3, 6], 1), ([0, 4, 4, 5], 3), ([0, 4, 4, 7], 3), ([0, 5, 4, 7], 1)):
        assert QC.ref(dict(c, link_off=np.uint64(off)))[:2] == (QR.INVALID_ARG, (link, QR.UMAX))
    # the smallest bad packet; ahead of an overflow at a smaller record
    pk = c["packet"].copy()
    pk[[3, 5]] = 3, 9
    free = c["free_in"].copy()
    free[0] = MAX - 20
    assert QC.ref(dict(c, packet=pk))[:2] == (QR.INVALID_ARG, (0, 3))
    assert QC.ref(dict(c, packet=pk, free_in=free))[:2] == (QR.INVALID_ARG, (0, 3))
    rc, pair, res = QC.ref(dict(c, free_in=free))  # MAX - 20 + 15 + 5 = MAX exactly at record 1
    assert (rc, pair) == (QR.TIME_OVERFLOW, (0, 1)) and int(res.done[0]) == MAX - 5 and int(res.done[1]) == MAX
    free[0] = MAX - 21
    assert QC.ref(dict(c, free_in=free))[:2] == (QR.TIME_OVERFLOW, (0, 2))


# ---- the cap on the real traces
def _table(O, g):
    nodes = np.arange(g["n"], dtype=np.uint32)
    rc, lat, loss, _ = O.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], nodes,
                                        rows=(0, g["n"]), threads=4)
    assert rc == 0
    pred, _, bad = R.tree_ref(g, nodes, (0, g["n"]), lat, loss)
    assert bad is None
    return nodes, lat, pred


def _capped(link_off, enter, packet, weight, cost):
    rc, _, res = QR.loop(link_off, enter, packet, weight, cost_ps=cost)
    assert rc == QR.OK
    deep, waits, gap = QC.conditions(link_off, res)
    assert deep, f"no record with ahead >= 64 (the most: {int(res.ahead.max())})"
    assert waits, "no link with a positive wait"
    assert gap, "no link with an idle gap after a wait"


@pytest.mark.parametrize("which", ["tie", "wide", "group"])
def test_round_conditions(oracle, which):
    """tie_round() and wide_round() as PathTree.link_queue_round takes them (every packet counted,
    payload weights); the tie round with queue_cases.group_status as Group.link_queue_round takes it
    (the members' batches concatenated: the same for every world size)."""
    g = XC.wide_graph() if which == "wide" else LC.tie_graph()
    nodes, lat, pred = _table(oracle, g)
    status = None
    if which == "wide":
        hosts, pk = XC.wide_round()
    else:
        hosts, pk, mixed = XC.tie_round()
        if which == "group":
            for world in QC.GROUP_WORLDS:
                cat, status, _ = GC.concat(GC.split(hosts, pk, QC.group_status(mixed), g["n"], world))
                assert world > 1 or all(np.array_equal(cat[k], pk[k]) for k in pk)
            pk = cat  # (of the last world: the counted packets are the same set in another order)
    tr = XR.trace(g, nodes, (0, g["n"]), pred, lat, hosts, pk, status)
    nl = XR.n_links(g)
    _capped(tr[0], tr[3], tr[1], pk["payload"], np.full(nl, QC.WIDE_COST if which == "wide" else QC.TIE_COST, np.uint64))


@pytest.mark.parametrize("name", WC.NAMES)
def test_sweep_conditions(oracle, name):
    c, r = WC.case(name), WC.refs(oracle, name)[0]
    assert c["views"][0]["rows"] == (0, c["g"]["n"])
    pk, status = QC.sweep_round(c)
    tr = XR.trace(c["g"], c["nodes"], (0, c["g"]["n"]), r["pred"], r["lat"], c["hosts"], pk, status)
    cost = QC.sweep_costs(name, XR.n_links(c["g"]))
    assert set(cost.tolist()) <= set(QC.COSTS)
    _capped(tr[0], tr[3], tr[1], pk["payload"], cost)


# ---- the layers
def test_exports():
    from shadow_amd import _capi

    assert "sg_link_queue" in _capi.EXPORTED
    so = os.path.join(ROOT, "shadow_amd", "libshadow_gpu.so")
    assert os.path.exists(so), "libshadow_gpu.so is not built"
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
        assert "sg_link_queue" in {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    else:  # the dynamic string table holds the name
        with open(so, "rb") as f:
            assert b"\0sg_link_queue\0" in f.read()


def test_python_callables():
    import shadow_amd
    from shadow_amd import Group, NetworkGraph, PathTree

    assert callable(shadow_amd.link_queue) and callable(getattr(NetworkGraph, "link_queue_device", None))
    assert callable(getattr(PathTree, "link_queue_round", None)) and callable(getattr(Group, "link_queue_round", None))
    assert shadow_amd.LinkQueueResult._fields == ("wait_ns", "done_ns", "ahead", "link_free", "link_busy_ns",
                                                  "link_wait_max_ns", "link_wait_sum_ns", "link_ahead_max")
    f = shadow_amd.cost_ps_from_bandwidth
    assert f(10**9) == 8000 and f(100 * 10**9) == 80 and f(10**9, unit_bytes=1500) == 12_000_000
    assert f(3 * 10**9) == 2667  # rounded up: a link is never faster than its rate
    assert f([10**9, 8 * 10**6]).tolist() == [8000, 10**6] and f([10**9]).dtype == np.uint64
    with pytest.raises(ValueError):
        f(0)
