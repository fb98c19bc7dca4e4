"""The link-time-series reference (tests/series_ref.py) on the hand graph of
test_trace_ref_cpu.py with every cell written out for both `at` values, its identity against the
per-packet link-load reference, the new entry points, and the conditions the GPU cases' inputs
must meet (test_series_gpu.py), asserted here so that the cases qualify by the references alone.
No GPU."""
import numpy as np
import pytest

import link_cases as LC
import link_ref as LR
import link_round_cases as RC
import link_round_ref as RR
import series_cases as SC
import series_ref as SR
import trace_cases as XC
import trace_ref as XR
import tree_ref as R


def _table(O, g, nodes=None, rows=None):
    nodes = np.arange(g["n"], dtype=np.uint32) if nodes is None else nodes
    rows = (0, g["n"]) if rows is None else rows
    rc, lat, loss, _ = O.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], nodes,
                                        rows=rows, threads=4)
    assert rc == 0
    pred, _, bad = R.tree_ref(g, nodes, rows, lat, loss)
    assert bad is None
    return nodes, rows, lat, loss, pred


def test_hand_graph(oracle):
    g = SC.hand_graph()
    _, _, keys = LR.links(g)
    nodes, rows, lat, _, pred = _table(oracle, g)
    assert pred[0].tolist() == [0, 0, 0, 2] and pred[1].tolist() == [1, 1, 1, 2] and pred[3].tolist() == [2, 2, 3, 3]
    k = lambda u, v: int(LR.link_index(keys, [u], [v])[0])  # noqa: E731
    nl = XR.n_links(g)
    assert nl == 12
    hosts, pk, status = SC.hand_round()
    T = SC.HAND_T
    # bins [T, T + 500), .. , [T + 1500, T + 2000); weights 1, 2, 4, 8, (16), 32.  The crossings:
    #   (0, 2): packet 5 (T - 200, T + 1300), packet 0 (T, T + 1500)
    #   (2, 3): packet 5 (T + 1300, T + 2300), packets 0 and 1 (T + 1500, T + 2500)
    #   (1, 2): packet 1 (T + 500, T + 1500)     (0, 0): packet 2 (T + 7, T + 1007)
    #   (3, 2): packet 3 (T + 100, T + 1100)     (2, 0): packet 3 (T + 1100, T + 2600)
    want = {SR.AT_ENTER: {k(0, 2): ([1, 0, 0, 0], 32, 0), k(2, 3): ([0, 0, 32, 3], 0, 0), k(1, 2): ([0, 2, 0, 0], 0, 0),
                          k(0, 0): ([4, 0, 0, 0], 0, 0), k(3, 2): ([8, 0, 0, 0], 0, 0), k(2, 0): ([0, 0, 8, 0], 0, 0)},
            SR.AT_EXIT: {k(0, 2): ([0, 0, 32, 1], 0, 0), k(2, 3): ([0, 0, 0, 0], 0, 35), k(1, 2): ([0, 0, 0, 2], 0, 0),
                         k(0, 0): ([0, 0, 4, 0], 0, 0), k(3, 2): ([0, 0, 8, 0], 0, 0), k(2, 0): ([0, 0, 0, 0], 0, 8)}}

    def cells(series, outside):
        assert series.dtype == outside.dtype == np.uint64 and outside.shape == (len(series), 2)
        return {s: (series[s].tolist(), int(outside[s, 0]), int(outside[s, 1])) for s in range(len(series))
                if series[s].any() or outside[s].any()}

    kw = dict(weight=pk["payload"], t0=T, bin_ns=500, n_bins=4)
    for at in (SR.AT_ENTER, SR.AT_EXIT):
        got = SR.series(g, nodes, rows, pred, lat, hosts, pk, status, at=at, **kw)
        assert got[0].shape == (nl, 4) and cells(*got) == want[at]
        # status = None: packet 4 (weight 16) counts, the twin of packet 0
        every = {L: (list(v[0]), v[1], v[2]) for L, v in want[at].items()}
        if at == SR.AT_ENTER:
            every[k(0, 2)][0][0] += 16
            every[k(2, 3)][0][3] += 16
        else:
            every[k(0, 2)][0][3] += 16
            every[k(2, 3)] = (every[k(2, 3)][0], 0, 35 + 16)
        assert cells(*SR.series(g, nodes, rows, pred, lat, hosts, pk, None, at=at, **kw)) == every
        # unit weights count crossings
        ones = SR.series(g, nodes, rows, pred, lat, hosts, pk, status, at=at, t0=T, bin_ns=500, n_bins=4)
        assert int(SR.slot_totals(*ones).sum()) == 9
        # a list of links: slot = position; the others are not watched
        two = [k(2, 3), k(0, 0)]
        m, ns = SR.list_slots(g, two)
        assert ns == 2 and m[two].tolist() == [0, 1] and int((m == SR.UMAX).sum()) == nl - 2
        assert cells(*SR.series(g, nodes, rows, pred, lat, hosts, pk, status, slot=m, n_slots=2, at=at, **kw)) == \
            {0: want[at][two[0]], 1: want[at][two[1]]}
        # both directions of an edge in one slot
        tail, head, _ = LR.links(g)
        m, ns = SC.both_directions(tail, head)
        assert ns == 8 and m[k(0, 2)] == m[k(2, 0)] and m[k(3, 2)] == m[k(2, 3)]
        got = cells(*SR.series(g, nodes, rows, pred, lat, hosts, pk, status, slot=m, n_slots=ns, at=at, **kw))
        a, b = want[at][k(0, 2)], want[at][k(2, 0)]
        assert got[int(m[k(0, 2)])] == ([x + y for x, y in zip(a[0], b[0])], a[1] + b[1], a[2] + b[2])
        # nothing watched; and the sums are added to a base
        none = np.full(nl, SR.UMAX, np.uint32)
        assert cells(*SR.series(g, nodes, rows, pred, lat, hosts, pk, status, slot=none, n_slots=3, at=at, **kw)) == {}
        base = SC.bases(nl, 4)
        got = SR.series(g, nodes, rows, pred, lat, hosts, pk, status, at=at, base=base, **kw)
        plain = SR.series(g, nodes, rows, pred, lat, hosts, pk, status, at=at, **kw)
        assert np.array_equal(got[0], plain[0] + SC.BASE_SERIES) and np.array_equal(got[1], plain[1] + SC.BASE_OUTSIDE)
        assert (base[0] == SC.BASE_SERIES).all()  # (the base itself is left alone)


@pytest.fixture(scope="module")
def tie(oracle):
    g = LC.tie_graph()
    nodes, rows, lat, loss, pred = _table(oracle, g)
    hosts, pk, mixed = XC.tie_round()
    return dict(g=g, nodes=nodes, lat=lat, pred=pred, hosts=hosts, pk=pk, mixed=mixed)


def test_identity(tie):
    """Per slot, the bins and the two outside cells sum to the per-packet link loads of the slot's
    links: either `at`, weights or none, the identity, a shared-slot map and a list."""
    g, nodes, hosts, pk = tie["g"], tie["nodes"], tie["hosts"], tie["pk"]
    tail, head, _ = LR.links(g)
    both = SC.both_directions(tail, head)
    some = SR.list_slots(g, [5, 17, 400, 401, XR.n_links(g) - 1])
    for status, weight in ((None, None), (tie["mixed"], pk["payload"]), (tie["mixed"], RC.big_weights(len(pk["src"])))):
        load = RR.link_load_round(g, nodes, (0, 300), tie["pred"], hosts, pk, status, weight)[0]
        cross = SR.crossings(g, nodes, (0, 300), tie["pred"], tie["lat"], hosts, pk, status, weight)
        for (slot, ns), at, (bin_ns, n_bins) in ((SR.identity_slots(g), SR.AT_ENTER, SC.BIN_SETS[0]),
                                                 (both, SR.AT_EXIT, SC.BIN_SETS[2]), (some, SR.AT_EXIT, SC.BIN_SETS[1])):
            got = SR.bin_crossings(cross, slot, ns, at, SC.TIE_T0, bin_ns, n_bins)
            assert np.array_equal(SR.slot_totals(*got), SR.slot_loads(load, slot, ns))
        if weight is not None and weight is not pk["payload"]:  # the big weights: cells pass 2^32
            wide = SR.bin_crossings(cross, None, XR.n_links(g), SR.AT_ENTER, SC.TIE_T0, *SC.BIN_SETS[1])[0]
            assert int((wide >= np.uint64(1 << 32)).sum()) > 100


def test_entry_points():
    from shadow_amd import _capi
    from shadow_amd.graph import NetworkGraph, PathTree, series_slots
    from shadow_amd.group import Group

    L = _capi.load()
    for sym in ("sg_link_series_packets", "sg_group_link_series_packets"):
        assert sym in _capi.EXPORTED and hasattr(L, sym), sym
    assert L.sg_abi_version() == 7
    assert callable(NetworkGraph.link_series_packets_device) and callable(PathTree.link_series_round)
    assert callable(Group.link_series_round)
    assert series_slots(None, 12) == (None, 12)
    m, ns = series_slots([7, 3], 12)
    assert ns == 2 and m.dtype == np.uint32 and m[7] == 0 and m[3] == 1 and int((m == 0xFFFFFFFF).sum()) == 10
    full = np.full(12, 0xFFFFFFFF, np.uint32)
    full[[1, 2]] = 4
    assert series_slots(full, 12)[1] == 5 and series_slots(full, 12)[0] is full
    for bad in ([12], [3, 3], []):
        with pytest.raises(ValueError):
            series_slots(bad, 12)


def test_case_conditions(tie, oracle):
    """The tie round's three bin sets place the crossings as the table says; no (link, 250 us bin)
    cell holds more than 20 crossings; the wide round's times pass 2^32; the quotient-edge rounds
    hold offsets whose truncated quotient would land inside; the budget shapes are 63, 64, 65 cells."""
    g, nodes, hosts, pk = tie["g"], tie["nodes"], tie["hosts"], tie["pk"]
    cross = SR.crossings(g, nodes, (0, 300), tie["pred"], tie["lat"], hosts, pk)
    link, _, enter, _ = cross
    assert len(link) == SC.TIE_CROSSINGS
    assert min(enter) == SC.T0 and max(enter) - SC.T0 == 11_750_000
    for (bin_ns, n_bins), (before, inside, after, edge) in SC.TIE_PLACES.items():
        got = SR.place_counts(cross, SR.AT_ENTER, SC.TIE_T0, bin_ns, n_bins)
        print(f"tie round, {bin_ns} ns x {n_bins}: before, inside, after, on an edge = {got}")
        assert got[:3] == (before, inside, after) and (edge is None or got[3] == edge)
    assert [tuple(k) for k in SC.TIE_PLACES] == [tuple(b) for b in SC.BIN_SETS]
    cells = SR.bin_crossings(cross, None, XR.n_links(g), SR.AT_ENTER, SC.T0, 250_000, 64)[0]
    assert 1 < int(cells.max()) <= 20
    # the wide round
    gw = XC.wide_graph()
    nodesw, rowsw, latw, _, predw = _table(oracle, gw)
    hw, wpk = XC.wide_round()
    _, _, enter, leave = SR.crossings(gw, nodesw, rowsw, predw, latw, hw, wpk)
    assert len(enter) == 36_365 and sum(t >= 1 << 32 for t in enter) == 34_003 and 5.4e10 < max(enter) < 5.6e10
    # the quotient edges
    for bin_ns in SC.EDGE_BINS:
        xs = SC.edge_offsets(bin_ns)
        _, epk = SC.edge_round(xs)
        assert [int(t) - SC.EDGE_T0 for t in epk["send_time"]] == xs and -1 in xs and (1 << 63) + 5 in xs
        for b in (1, 2, 63, 64, SC.EDGE_N_BINS - 1, SC.EDGE_N_BINS):
            assert b * bin_ns - 1 in xs and b * bin_ns in xs
        wrapped = [x for x in xs if x >= 0 and x // bin_ns >= 1 << 32 and (x // bin_ns) % (1 << 32) < SC.EDGE_N_BINS]
        assert len(wrapped) >= (4 if bin_ns <= 1 << 20 else 0), bin_ns
    for bin_ns, n_bins in SC.PAST_BINS:
        assert SC.PAST_T0 + n_bins * bin_ns > 1 << 64
        _, ppk = SC.edge_round(list(SC.PAST_OFFSETS), SC.PAST_T0)
        assert int(ppk["send_time"][-1]) + 2 * SC.MS == SC.LAST
    assert [s * (b + 2) for s, b in SC.BUDGET_SHAPES] == [63, 64, 65]
    # the hot cell: every crossing of a link of the tier round at one time
    gt = XC.tier_graph()
    nodes3, rows3, lat3, _, pred3 = _table(oracle, gt, rows=(0, 1))
    for n in (1, 64, 65, 2049):
        ht, tpk = XC.tier_round(n, False)
        s = SR.series(gt, nodes3, rows3, pred3, lat3, ht, tpk, t0=SC.T0, bin_ns=SC.MS, n_bins=4)
        assert sorted(s[0][s[0] > 0].tolist()) == [n, n] and not s[1].any()
