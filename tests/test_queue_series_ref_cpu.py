"""The link-queue series' reference (tests/queue_series_ref.py) and cases, qualified without a GPU: the
two restatements agree, the identities of include/shadow_gpu.h hold on the reference, a session's
rounds sum to the single carried call, the constant is where it must be and the Python surface checks
its arguments."""
import os
import re

import numpy as np
import pytest

import outcomes_cases as OC
import queue_carry_cases as CC
import queue_cases as QC
import queue_drop_cases as DC
import queue_series_cases as SC
import queue_series_ref as SR
import queue_window_cases as WC
import queue_window_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX = SR.MAX


def both(c, out, hdr, **kw):
    nl = len(c["link_off"]) - 1
    terms = SR.terms_of(c, out, hdr, **kw)
    a, b = SR.naive(terms, hdr, nl), SR.diffs(terms, hdr, nl)
    assert a.shape == b.shape and np.array_equal(a, b)
    return a


def check_identities(c, out, hdr, M, drop=False):
    """Plane 0 sums to busy, plane 1 to wait_sum; with unit weights plane 3 to the drops, plane 2 to the
    number served."""
    nl = len(c["link_off"]) - 1
    sums = SR.plane_sums(M)
    assert sums[0] == SR.link_sums_by_slot(out["busy"][:nl], hdr, nl)
    assert sums[1] == SR.link_sums_by_slot(out["wait_sum"], hdr, nl)
    if c["weight"] is None or (np.asarray(c["weight"]) == 1).all():
        n = len(c["enter"])
        off = c["link_off"].astype(np.int64)
        served = np.asarray(out["wait"][:n]) != np.uint64(MAX)
        per_link = [int(served[off[k]:off[k + 1]].sum()) for k in range(nl)]
        assert sums[2] == SR.link_sums_by_slot(per_link, hdr, nl)
        if drop:
            assert sums[3] == SR.link_sums_by_slot(out["ahead_max"][nl:], hdr, nl)


def test_hand_example():
    """queue_cases.hand(): link 0 (free from 5) serves [10, 25) [25, 30) [30, 32) [32, 37), the waits are
    [11, 25) and [30, 32); link 2 (free from 100) serves [100, 110) [110, 120), waits [40, 100) [50, 110)."""
    c, want = QC.hand()
    out = {k: getattr(want, k) for k in want._fields}
    hdr = SR.header(10, 10, 3)  # bins [10, 20) [20, 30) [30, 40)
    M = both(c, out, hdr)
    assert M[0, 0].tolist() == [10, 10, 7, 0, 0] and M[1, 0].tolist() == [9, 5, 2, 0, 0]
    assert M[2, 0].tolist() == [0, 10, 1 + 3 + 3, 0, 0]  # weights: packet 2, 0, 1, 0 -> 10, 3, 1, 3, at done 25, 30, 32, 37
    assert M[:, 1].sum() == 0
    assert M[0, 2].tolist() == [0, 0, 0, 0, 20] and M[1, 2].tolist() == [0, 0, 0, 0, 120] and M[2, 2].tolist() == [0, 0, 0, 0, 20]
    assert M[3].sum() == 0
    check_identities(c, out, hdr, M)


@pytest.mark.parametrize("k", range(len(SC.EDGES)), ids=[e[0] for e in SC.EDGES])
def test_edges_one_by_one(k):
    c = SC.edges([k])
    out = SC.first_order_out(c)
    _, e, start, s = SC.EDGES[k]
    assert int(out["wait"][0]) == start - e and int(out["done"][0]) == start + s
    for t0, bin_ns, B in ((SC.T0, SC.BIN, SC.BINS), (SC.T0, 1, 40), (SC.T0, 40, 1), (0, 1 << 40, 2), (MAX - 20, 7, 5)):
        hdr = SR.header(t0, bin_ns, B)
        check_identities(c, out, hdr, both(c, out, hdr))


def test_edges_values():
    c = SC.edges()
    out = SC.first_order_out(c)
    hdr = SR.header(SC.T0, SC.BIN, SC.BINS)
    M = both(c, out, hdr)
    name = [e[0] for e in SC.EDGES]
    row = lambda plane, what: M[plane, name.index(what)].tolist()  # noqa: E731
    assert row(1, "inside one bin") == [3, 0, 0, 0, 0, 0] and row(0, "inside one bin") == [4, 0, 0, 0, 0, 0]
    assert row(1, "across exactly two bins") == [5, 5, 0, 0, 0, 0] and row(0, "across exactly two bins") == [0, 5, 5, 0, 0, 0]
    assert row(1, "ending exactly on a bin edge") == [7, 0, 0, 0, 0, 0] and row(0, "ending exactly on a bin edge") == [0, 10, 0, 0, 0, 0]
    assert row(0, "of length 0, both") == row(1, "of length 0, both") == [0] * 6
    assert row(2, "of length 0 on a bin edge") == [0] * 6  # (weight 0)
    assert row(1, "wait across t0") == [5, 0, 0, 0, 10, 0] and row(0, "service across t0") == [5, 0, 0, 0, 5, 0]
    assert row(1, "wait across the end") == [0, 0, 0, 10, 0, 5] and row(0, "service across the end") == [0, 0, 0, 5, 0, 5]
    assert row(1, "wholly before") == [0, 0, 0, 0, 50, 0] and row(0, "ending exactly at t0") == [0, 0, 0, 0, 50, 0]
    assert row(1, "wholly after") == [0, 0, 0, 0, 0, 50] and row(0, "starting exactly at the end") == [0, 0, 0, 0, 0, 7]
    assert row(1, "wait covering the whole range") == [10, 10, 10, 10, 100, 60]
    assert row(0, "service covering the whole range") == [10, 10, 10, 10, 50, 110]
    assert row(0, "three whole bins between two partial ones") == [5, 10, 10, 8, 0, 0]
    assert row(0, "whole bins only") == [0, 10, 10, 10, 0, 0]
    check_identities(c, out, hdr, M)


def test_end_past_the_range():
    """t0 + B bin_ns >= 2^64: the decision is by the quotient; times near 2^63."""
    c = QC.case([0, 2], [(1 << 63) - 5, (1 << 63) + 1], None, None, [3000], [1 << 63])
    out = SC.first_order_out(c)
    for hdr in (SR.header((1 << 63) - 8, 1 << 62, 3), SR.header(1 << 63, 1 << 60, 16), SR.header((1 << 63) + 2, 3, 2)):
        assert int(hdr[0]) + int(hdr[1]) * int(hdr[2]) >= (1 << 64) or int(hdr[1]) == 3
        check_identities(c, out, hdr, both(c, out, hdr))


@pytest.mark.parametrize("seed", range(6))
def test_random_first_order(seed):
    rng = np.random.default_rng(seed)
    c = QC.random_trace(rng.integers(0, 40, 7).tolist(), seed, free_max=30)
    c = DC.draw_limits(c, seed + 50)
    nl = 7
    slots = [int(rng.integers(0, 3)) if rng.random() < 0.7 else SR.UNWATCHED for _ in range(nl)]
    for drop in (False, True):
        out = SC.first_order_out(c, drop)
        for hdr in (SR.header(1000, 25, 12), SR.header(1100, 7, 31, slots, 3), SR.header(0, 1 << 20, 1, slots)):
            M = both(c, out, hdr, drop=drop)
            check_identities(c, out, hdr, M, drop)
            if drop:
                assert M[3].sum() > 0 or not int(np.asarray(out["ahead_max"][nl:]).sum())


@pytest.mark.parametrize("seed", range(4))
def test_random_carried_and_windowed(seed):
    c = OC.with_base(DC.draw_limits(CC.random_chains(seed), seed + 9), 10**6)
    nl = len(c["link_off"]) - 1
    for drop in (False, True):
        for H in WC.horizons(c, drop):
            out = SC.carried_out(c, H, drop, True)
            hdr = SC.span_header(c, SC.carried_out(c, MAX, drop), 9, margin=1)
            M = both(c, out, hdr, drop=drop, window=True)
            check_identities(c, out, hdr, M, drop)
            if H == MAX:
                assert np.array_equal(M, both(c, out, hdr, drop=drop))  # (no record is pending)


def test_one_link_slot_is_at_most_busy():
    """From a zeroed matrix a slot of one link has M[0][s][c] <= bin_ns in every bin."""
    c = QC.random_trace([300, 0, 120], 5, free_max=10)
    out = SC.first_order_out(c)
    assert int(out["wait_max"].max()) > 0
    for bin_ns, B in ((1, 3000), (13, 300), (1000, 5)):
        hdr = SR.header(990, bin_ns, B)
        M = SR.diffs(SR.terms_of(c, out, hdr), hdr, 3)
        assert int(M[0, :, :B].max()) <= bin_ns and int(M[0, :, :B].max()) > 0


@pytest.mark.parametrize("k", (1, 2, 5, 17))
@pytest.mark.parametrize("drop", (False, True), ids=("plain", "drop"))
def test_session_sums_to_the_single_call(k, drop):
    """The matrices of a session's re-fed calls, the last at H = 2^64 - 1, sum to the matrix of one
    carried call over the whole trace, bit for bit."""
    c = WC.segments(40)
    nl = len(c["link_off"]) - 1
    slots = [0, 1, 1, SR.UNWATCHED]
    whole_out = SC.carried_out(c, MAX, drop)
    hdr = SC.span_header(c, whole_out, 11, slots, 2, margin=1)
    total = np.zeros((4, 2, 13), np.uint64)
    calls = []

    def solve(rc, H, d):
        out = WR.define(rc, H, d, True)[1]
        calls.append(H)
        total[...] = SC.matrix(rc, out, hdr, drop=d, window=True, start=total, form=SR.naive)
        return out

    whole, _ = WC.run_session(c, k, 7, drop, solve)
    assert len(calls) == k + 1 and calls[-1] == MAX
    want = SC.matrix(whole, SC.carried_out(whole, MAX, drop), hdr, drop=drop, form=SR.naive)
    assert want[:2].sum() > 0 and np.array_equal(total, want)
    assert nl == 4


def test_constant():
    from shadow_amd import _capi

    flag = SR.SERIES_FLAG
    assert getattr(_capi, flag) == SR.SERIES == 0x40
    with open(_capi.HEADER_PATH) as f:
        assert re.search(rf"^#define {flag} 0x40u$", f.read(), flags=re.M)
    with open(os.path.join(ROOT, "bindings", "shadow-gpu-sys", "src", "lib.rs")) as f:
        assert re.search(rf"^pub const {flag}: u32 = 64;$", f.read(), flags=re.M)


def test_python_surface():
    import inspect

    import shadow_amd
    from shadow_amd import Group, LinkQueueSeries, LinkQueueSession, NetworkGraph, PathTree

    assert "LinkQueueSeries" in shadow_amd.__all__
    for f in (shadow_amd.link_queue, NetworkGraph.link_queue_device, PathTree.link_queue_round, Group.link_queue_round,
              LinkQueueSession.__init__):
        p = inspect.signature(f).parameters["series"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    sig = inspect.signature(LinkQueueSeries.__init__).parameters
    assert list(sig)[1:5] == ["ctx_or_graph", "t0_ns", "bin_ns", "n_bins"]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("n_links", "link_slot", "n_slots", "watch", "device"))
    s = LinkQueueSeries(None, 5, 10, 3, n_links=4, watch=[3, 1])
    assert s.n_slots == 2 and s.link_slot.tolist() == [MAX, 0, MAX, 1] and s.cells == 10
    assert s.busy_ns.shape == (2, 3) and s.before.shape == (4, 2) and s.utilisation().dtype == np.float64
    assert LinkQueueSeries(None, 0, 1, 1, n_links=3).n_slots == 3
    s = LinkQueueSeries(None, 0, 1, 1, n_links=3, link_slot=[2, -1, 2])
    assert s.n_slots == 3 and s.link_slot.tolist() == [2, MAX, 2]
    for kw in (dict(bin_ns=0), dict(n_bins=0), dict(n_bins=1 << 32), dict(t0_ns=-1), dict(watch=[0, 0]), dict(watch=[4]),
               dict(watch=[]), dict(link_slot=[0, 1]), dict(link_slot=[0, 1, 2, 3], n_slots=3), dict(watch=[1], link_slot=[0] * 4),
               dict(n_slots=2), dict(n_bins=(1 << 31) // 4), dict(n_links=None)):
        args = dict(dict(t0_ns=0, bin_ns=1, n_bins=2, n_links=4), **kw)
        with pytest.raises(ValueError):
            LinkQueueSeries(None, args.pop("t0_ns"), args.pop("bin_ns"), args.pop("n_bins"), **args)
    with pytest.raises(ValueError):
        LinkQueueSeries(None, 0, 1, 1, n_links=3)._check(4)
