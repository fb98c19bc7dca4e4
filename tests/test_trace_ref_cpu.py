"""The link-trace reference (tests/trace_ref.py) on a hand graph with every record written out,
its conservation laws against the per-packet link-load and hop-record references, the oracle's
delivery times, and the conditions the GPU cases' inputs must meet (test_trace_gpu.py), checked
here so that the inputs qualify by the references alone.  No GPU."""
import numpy as np
import pytest

import link_cases as LC
import link_ref as LR
import link_round_cases as RC
import link_round_ref as RR
import paths_ref as PR
import trace_cases as XC
import trace_ref as XR
import tree_ref as R
from shadow_amd import synth


def _table(O, g, nodes=None, rows=None):
    nodes = np.arange(g["n"], dtype=np.uint32) if nodes is None else nodes
    rows = (0, g["n"]) if rows is None else rows
    rc, lat, loss, _ = O.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], nodes,
                                        rows=rows, threads=4)
    assert rc == 0
    pred, _, bad = R.tree_ref(g, nodes, rows, lat, loss)
    assert bad is None
    return nodes, rows, lat, loss, pred


def _hand_graph():
    """The path 0 - 1 - 2 - 3 with 1 us arcs and self-loops, and the chord 0 - 2 of 1.5 us: from
    node 0, nodes 2 and 3 are reached over the chord."""
    edges = [(0, 1, 1000), (1, 2, 1000), (2, 3, 1000), (0, 2, 1500)]
    src = list(range(4)) + [e[0] for e in edges]
    dst = list(range(4)) + [e[1] for e in edges]
    lat = [1000] * 4 + [e[2] for e in edges]
    return dict(n=4, src=np.uint32(src), dst=np.uint32(dst), lat=np.uint64(lat), loss=np.zeros(8, np.float32),
                directed=False)


def test_hand_graph(oracle):
    g = _hand_graph()
    _, _, keys = LR.links(g)
    nodes, rows, lat, _, pred = _table(oracle, g)
    assert pred[0].tolist() == [0, 0, 0, 2] and pred[1].tolist() == [1, 1, 1, 2] and pred[3].tolist() == [2, 2, 3, 3]
    k = lambda u, v: int(LR.link_index(keys, [u], [v])[0])
    nl = XR.n_links(g)
    assert nl == 12
    # host h on node h, host 4 on node 0.  (sender, receiver, send time, status):
    T = 10_000
    sends = [(0, 3, T, 0),        # 0 - 2 - 3
             (1, 3, T + 500, 0),  # 1 - 2 - 3: enters (2, 3) when packet 0 does
             (0, 4, T + 7, 0),    # to its own node: the self-loop
             (3, 0, T + 100, 0),  # 3 - 2 - 0
             (0, 3, T, 1),        # dropped: no record
             (0, 3, T - 200, 0)]  # 0 - 2 - 3 ahead of packet 0
    hosts = synth.make_hosts(5, 4)
    pk = dict(src=np.uint32([s[0] for s in sends]), dst_ip=hosts["ip"][[s[1] for s in sends]],
              send_time=np.uint64([s[2] for s in sends]))
    status = np.uint8([s[3] for s in sends])
    want = {k(0, 2): [(5, 1, T - 200, T + 1300), (0, 1, T, T + 1500)],
            k(2, 3): [(5, 2, T + 1300, T + 2300), (0, 2, T + 1500, T + 2500), (1, 2, T + 1500, T + 2500)],
            k(1, 2): [(1, 1, T + 500, T + 1500)],
            k(0, 0): [(2, 1, T + 7, T + 1007)],
            k(3, 2): [(3, 1, T + 100, T + 1100)],
            k(2, 0): [(3, 2, T + 1100, T + 2600)]}

    def segments(out):
        off, packet, hop, enter, leave = out
        assert off.dtype == enter.dtype == leave.dtype == np.uint64 and packet.dtype == hop.dtype == np.uint32
        assert len(off) == nl + 1 and off[0] == 0 and int(off[-1]) == len(packet) == len(hop) == len(enter) == len(leave)
        return {L: list(zip(packet[a:b].tolist(), hop[a:b].tolist(), enter[a:b].tolist(), leave[a:b].tolist()))
                for L, (a, b) in enumerate(zip(off[:-1].astype(int), off[1:].astype(int))) if b > a}

    assert segments(XR.trace(g, nodes, rows, pred, lat, hosts, pk, status)) == want
    # status = None: packet 4 counts, the twin of packet 0; on (2, 3) packet 1 ties with both and lies between
    every = {L: list(v) for L, v in want.items()}
    every[k(0, 2)].append((4, 1, T, T + 1500))
    every[k(2, 3)].append((4, 2, T + 1500, T + 2500))
    assert segments(XR.trace(g, nodes, rows, pred, lat, hosts, pk, None)) == every
    # watch: a mask, or link numbers
    two = [k(2, 3), k(0, 0)]
    mask = np.zeros(nl, np.uint8)
    mask[two] = 1
    for watch in (mask, mask.astype(bool), two, np.array(two)):
        assert segments(XR.trace(g, nodes, rows, pred, lat, hosts, pk, status, watch)) == {L: want[L] for L in two}
    assert XR.trace(g, nodes, rows, pred, lat, hosts, pk, status, np.zeros(nl, np.uint8))[0].tolist() == [0] * (nl + 1)
    # the overflow kind: the smallest counted packet whose arrival passes 2^64 - 1
    assert XR.first_overflow(nodes, rows, lat, hosts, pk, status) is None
    late = dict(pk, send_time=pk["send_time"].copy())
    late["send_time"][[1, 4, 5]] = np.uint64((1 << 64) - 2500), np.uint64((1 << 64) - 1), np.uint64((1 << 64) - 2000)
    assert int(lat[1, 3]) == 2000 and int(lat[0, 3]) == 2500
    assert XR.first_overflow(nodes, rows, lat, hosts, late, status) == 5  # (1: 2^64 - 500 fits; 4 does not count)
    assert XR.first_overflow(nodes, rows, lat, hosts, late, None) == 4


@pytest.fixture(scope="module")
def tie(oracle):
    g = LC.tie_graph()
    nodes, rows, lat, loss, pred = _table(oracle, g)
    hosts, pk, mixed = XC.tie_round()
    # the round's statuses, from the oracle's delivery round on the hosts' own streams
    rng = np.stack([oracle.xoshiro_seed(int(s)) for s in hosts["seed"]])
    ctr = np.zeros(hosts["n"], np.uint64)
    out = oracle.deliver_round(RC.ROUND_END, 2**63, 0, pk["src"], pk["dst_ip"], pk["payload"], pk["send_time"],
                               hosts["ip"], hosts["route"], lat, loss, rng, ctr)
    return dict(g=g, nodes=nodes, lat=lat, loss=loss, pred=pred, hosts=hosts, pk=pk, mixed=mixed, round=out)


def test_conservation(tie):
    """Records per link = the per-packet link loads with unit weights; the (packet, link, hop)
    triples = the transpose of the hop records; the last hop's exit = the oracle's delivery time."""
    g, pk, nodes, hosts = tie["g"], tie["pk"], tie["nodes"], tie["hosts"]
    for status in (tie["round"]["status"], None, tie["mixed"]):
        off, packet, hop, enter, leave = XR.trace(g, nodes, (0, 300), tie["pred"], tie["lat"], hosts, pk, status)
        want_l, _, hops = RR.link_load_round(g, nodes, (0, 300), tie["pred"], hosts, pk, status)
        assert np.array_equal(np.diff(off.astype(np.int64)).astype(np.uint64), want_l)
        poff, _, plink, plat, _ = PR.packet_records(g, nodes, (0, 300), tie["pred"], tie["lat"], tie["loss"], hosts, pk, status)
        cnt = np.diff(poff.astype(np.int64))
        ppacket = np.repeat(np.arange(len(cnt)), cnt)
        phop = np.arange(len(plink)) - np.repeat(poff[:-1].astype(np.int64), cnt) + 1
        got = np.stack([packet.astype(np.int64), XR.segment_links(off), hop.astype(np.int64)])
        want = np.stack([ppacket, plink.astype(np.int64), phop])
        assert np.array_equal(got[:, np.lexsort(got[::-1])], want[:, np.lexsort(want[::-1])])
        # (packet, hop) indexes the hop records: the same link, and the exit is the record's latency past the send
        at = poff[packet].astype(np.int64) + hop.astype(np.int64) - 1
        assert np.array_equal(plink[at].astype(np.int64), XR.segment_links(off))
        assert np.array_equal(leave, pk["send_time"][packet] + plat[at])
        assert (enter < leave).all()
        # the last hop of every counted packet
        last = hop == np.where(hops == RC.UMAX, 0, hops)[packet]
        assert int(last.sum()) == int((hops != RC.UMAX).sum()) and len(np.unique(packet[last])) == int(last.sum())
        if status is tie["round"]["status"]:
            assert 0 < int(last.sum()) == tie["round"]["delivered"]
            assert np.array_equal(np.maximum(leave[last], np.uint64(RC.ROUND_END)), tie["round"]["deliver_time"][packet[last]])


def test_case_conditions(tie, oracle):
    """(a): every record shares its enter time with another record of its link, under the mixed
    statuses and under none.  (b): the tier cases' segment lengths are the list, exactly.  (f):
    latencies past 2^32 ns, and a link whose enter times lie on both sides of 2^32.  (m): the
    paths with 2,047, 2,048 and 2,049 links."""
    g, pk, nodes = tie["g"], tie["pk"], tie["nodes"]
    assert len(pk["src"]) == 10000
    for status in (tie["mixed"], None):
        off, packet, _, enter, _ = XR.trace(g, nodes, (0, 300), tie["pred"], tie["lat"], tie["hosts"], pk, status)
        key = np.stack([XR.segment_links(off).astype(np.uint64), enter])
        _, inverse, counts = np.unique(key, axis=1, return_inverse=True, return_counts=True)
        shared = counts[np.ravel(inverse)]
        print(f"case (a): {len(packet)} records, {int((np.diff(off.astype(np.int64)) > 0).sum())} links in use, "
              f"longest segment {int(np.diff(off.astype(np.int64)).max())}, keys shared by {int(shared.min())} .. {int(shared.max())}")
        assert len(packet) > 10000 and int(shared.min()) >= 2
    gt = XC.tier_graph()
    nodes3, rows3, lat3, _, pred3 = _table(oracle, gt, rows=(0, 1))
    _, _, keys = LR.links(gt)
    l01, l12 = (int(LR.link_index(keys, [u], [v])[0]) for u, v in ((0, 1), (1, 2)))
    seen = []
    lengths = XC.tier_lengths(XC.PIECE) + XC.tier_lengths(XC.PIECE_DEFAULT)[-3:]
    for n in lengths:
        for shuffled in (False, True):
            hosts, tpk = XC.tier_round(n, shuffled)
            off, packet, hop, enter, _ = XR.trace(gt, nodes3, rows3, pred3, lat3, hosts, tpk)
            cnt = np.diff(off.astype(np.int64))
            assert sorted(np.flatnonzero(cnt).tolist()) == sorted([l01, l12]) and cnt[l01] == cnt[l12] == n
            a = int(off[l01])
            if shuffled:
                assert len(np.unique(tpk["send_time"])) == n and (np.diff(enter[a:a + n].astype(np.int64)) > 0).all()
                assert n < 3 or not (np.diff(packet[a:a + n].astype(np.int64)) > 0).all()
            else:
                assert np.array_equal(packet[a:a + n], np.arange(n)) and len(np.unique(enter[a:a + n])) == 1
        seen.append(n)
    assert seen == [1, 63, 64, 65, 127, 128, 129, 257, 383, 2049, 4097, 6143]
    # (m): the link counts, the written-out rows against the tree reference, no packet to its
    # sender's own node, sources spread along the path, and links in use in the tile's last counters
    for nl, (n, loops) in XC.SCAN_EDGE.items():
        ge = XC.scan_edge_graph(n, loops)
        assert XR.n_links(ge) == nl == 2 * (n - 1) + loops
        nodes_e, hosts, epk = XC.scan_edge_round(n)
        rows_e = (0, XC.SCAN_EDGE_ROWS)
        assert sorted(nodes_e.tolist()) == list(range(n))
        pred_e, lat_e = XC.scan_edge_tables(nodes_e)
        ref_pred, _, bad = R.tree_ref(ge, nodes_e, rows_e, lat_e, np.zeros(lat_e.shape, np.float32))
        assert bad is None and np.array_equal(ref_pred, pred_e)
        _, ri, cj = RR.counted_pairs(hosts, epk, None)
        assert len(ri) == 500 and (ri != cj).all() and int(ri.max()) < XC.SCAN_EDGE_ROWS
        src_nodes = np.unique(nodes_e[ri])
        assert int(src_nodes.min()) < n // 8 and int(src_nodes.max()) > n - n // 8 and len(src_nodes) == XC.SCAN_EDGE_ROWS
        off = XR.trace(ge, nodes_e, rows_e, pred_e, lat_e, hosts, epk)[0]
        cnt = np.diff(off.astype(np.int64))
        assert cnt[:8].any() and cnt[2040:].any() and int(cnt.max()) > 64
    gw = XC.wide_graph()
    nodesw, rowsw, latw, _, predw = _table(oracle, gw)
    hosts, wpk = XC.wide_round()
    off, _, _, enter, _ = XR.trace(gw, nodesw, rowsw, predw, latw, hosts, wpk)
    assert int(latw.max()) > 1 << 32 and XR.first_overflow(nodesw, rowsw, latw, hosts, wpk) is None
    links = XR.segment_links(off)
    below = np.bincount(links[enter < np.uint64(1 << 32)], minlength=len(off) - 1)
    above = np.bincount(links[enter >= np.uint64(1 << 32)], minlength=len(off) - 1)
    assert ((below > 0) & (above > 0)).sum() >= 10
