"""The per-packet link-load reference (tests/link_round_ref.py) on a hand graph with loads, bytes
and hops written out, its conservation law, and the conditions the GPU cases' inputs must meet
(test_link_round_gpu.py), checked here so that the inputs qualify by the references alone.  The
built library must export the new entry point.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import link_cases as LC
import link_ref as LR
import link_round_cases as RC
import link_round_ref as RR
import tree_ref as R
from shadow_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(O, g, nodes=None, rows=None):
    nodes = np.arange(g["n"], dtype=np.uint32) if nodes is None else nodes
    rows = (0, g["n"]) if rows is None else rows
    rc, lat, loss, _ = O.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], nodes,
                                        rows=rows, threads=4)
    assert rc == 0
    return nodes, rows, lat, loss


def _trees(O, g, nodes=None, rows=None):
    """pred rows (tests/tree_ref.py) from the oracle's table."""
    nodes, rows, lat, loss = _table(O, g, nodes, rows)
    pred, _, bad = R.tree_ref(g, nodes, rows, lat, loss)
    assert bad is None
    return pred


def _hand_graph():
    """A tree plus one chord and a parallel pair, 1 us arcs except the chord:
           0 - 1 - 3        1 = 1 (two edges)     4 - 5 costs 9 us (never on a shortest path)
           |   |
           2   4            2 - 5
    """
    edges = [(0, 1, 1), (0, 1, 1), (0, 2, 1), (1, 3, 1), (1, 4, 1), (2, 5, 1), (4, 5, 9)]
    src = list(range(6)) + [a for a, _, _ in edges]
    dst = list(range(6)) + [b for _, b, _ in edges]
    lat = [1000] * 6 + [1000 * w for _, _, w in edges]
    return dict(n=6, src=np.uint32(src), dst=np.uint32(dst), lat=np.uint64(lat), loss=np.zeros(len(src), np.float32),
                directed=False)


def test_hand_graph(oracle):
    g = _hand_graph()
    _, _, keys = LR.links(g)
    pred = _trees(oracle, g)
    assert pred[0].tolist() == [0, 0, 0, 1, 1, 2]
    hosts = synth.make_hosts(7, 6)  # host h on node h, host 6 on node 0
    # (source host, destination host, bytes, status)
    sends = [(0, 3, 100, 0), (0, 5, 50, 0), (0, 6, 7, 0), (3, 5, 1000, 0), (0, 3, 11, 1), (0, 3, 1, 0)]
    pk = dict(src=np.uint32([s for s, _, _, _ in sends]), dst_ip=hosts["ip"][[d for _, d, _, _ in sends]])
    w = np.uint32([b for _, _, b, _ in sends])
    status = np.uint8([st for _, _, _, st in sends])
    k = lambda u, v: int(LR.link_index(keys, [u], [v])[0])
    nodes = np.arange(6)
    # packets: 0 - 1 - 3 twice, 0 - 2 - 5, the self-loop of node 0, and 3 - 1 - 0 - 2 - 5
    link, node, hops = RR.link_load_round(g, nodes, (0, 6), pred, hosts, pk, status)
    want = np.zeros(18, np.uint64)
    want[[k(0, 1), k(1, 3), k(0, 2), k(2, 5)]] = 2
    want[[k(0, 0), k(3, 1), k(1, 0)]] = 1
    assert np.array_equal(link, want)
    assert node.tolist() == [1, 3, 2, 2, 0, 2]
    assert hops.tolist() == [2, 2, 1, 4, 0xFFFFFFFF, 2]
    # bytes
    link, node, hops2 = RR.link_load_round(g, nodes, (0, 6), pred, hosts, pk, status, w)
    want = np.zeros(18, np.uint64)
    want[[k(0, 1), k(1, 3)]] = 101
    want[[k(0, 2), k(2, 5)]] = 1050
    want[k(0, 0)] = 7
    want[[k(3, 1), k(1, 0)]] = 1000
    assert np.array_equal(link, want)
    assert node.tolist() == [1000, 1101, 1050, 101, 0, 1050]
    assert np.array_equal(hops, hops2)
    # every packet: the dropped one counts too
    link, _, hops = RR.link_load_round(g, nodes, (0, 6), pred, hosts, pk, None, w)
    assert link[k(0, 1)] == 112 and hops[4] == 2
    # what a bad input reports
    assert RR.first_bad_packet(hosts, pk, status, (0, 6), 6) is None
    assert RR.first_bad_packet(hosts, pk, status, (0, 3), 6) == 3  # host 3's row lies outside
    far = dict(pk, dst_ip=pk["dst_ip"].copy())
    far["dst_ip"][4] = far["dst_ip"][5] = 12345
    assert RR.first_bad_packet(hosts, far, status, (0, 6), 6) == 5  # packet 4 does not count
    assert RR.first_bad_packet(hosts, far, None, (0, 6), 6) == 4
    assert RR.first_bad_pred(g, nodes, (0, 6), pred, hosts, pk, status) is None
    p = pred.copy()
    p[3, 2] = 4  # (4, 2) is not a link: row 3's walk from node 5 fails at node 2
    assert RR.first_bad_pred(g, nodes, (0, 6), p, hosts, pk, status) == (3, 2)
    p = pred.copy()
    p[3, 0], p[3, 1] = 1, 0  # a 2-cycle under row 3's walk from node 5: its destination column
    assert RR.first_bad_pred(g, nodes, (0, 6), p, hosts, pk, status) == (3, 5)
    p = pred.copy()
    p[0, 4] = 99  # no packet crosses node 4
    assert RR.first_bad_pred(g, nodes, (0, 6), p, hosts, pk, status) is None


@pytest.fixture(scope="module")
def tie(oracle):
    g = LC.tie_graph()
    nodes, rows, lat, loss = _table(oracle, g)
    pred, _, bad = R.tree_ref(g, nodes, rows, lat, loss)
    assert bad is None
    hosts, pk = RC.tie_round()
    # the round's statuses, from the oracle's delivery round on the hosts' own streams
    rng = np.stack([oracle.xoshiro_seed(int(s)) for s in hosts["seed"]])
    ctr = np.zeros(hosts["n"], np.uint64)
    out = oracle.deliver_round(RC.ROUND_END, 2**63, 0, pk["src"], pk["dst_ip"], pk["payload"], pk["send_time"],
                               hosts["ip"], hosts["route"], lat, loss, rng, ctr)
    return dict(g=g, nodes=nodes, pred=pred, hosts=hosts, pk=pk, status=out["status"])


def test_conservation(tie):
    """The weighted hops of the counted packets equal the sum of the link increments, and the
    node increments are those of the links that are no self-loops."""
    g, pk = tie["g"], tie["pk"]
    tail, head, _ = LR.links(g)
    for status, weight in ((tie["status"], None), (tie["status"], pk["payload"]), (None, pk["payload"])):
        link, node, hops = RR.link_load_round(g, tie["nodes"], (0, 300), tie["pred"], tie["hosts"], pk, status, weight)
        c = hops != RC.UMAX
        w = np.ones(len(hops), np.int64) if weight is None else weight.astype(np.int64)
        assert int((w[c] * hops[c].astype(np.int64)).sum()) == int(link.sum())
        assert int(node.sum()) == int(link[tail != head].sum())
        if status is not None:
            assert np.array_equal(c, status == RC.DELIVERED)


def test_case_a_conditions(tie):
    """(a): measured 36 same-node packets among 12,377 counted; 1,832 (14.8 %) share their pair."""
    hosts, pk, status = tie["hosts"], tie["pk"], tie["status"]
    idx, ri, cj = RR.counted_pairs(hosts, pk, status)
    assert 0 < len(idx) < len(status)  # some are dropped
    same = int((ri == cj).sum())
    _, inv, cnt = np.unique(ri * 300 + cj, return_inverse=True, return_counts=True)
    shared = int((cnt[inv] > 1).sum())
    print(f"case (a): {len(idx)} counted, {same} same-node, {shared} share their pair")
    assert same >= 10 and shared >= 0.05 * len(idx)


def test_case_b_conditions(tie):
    """(b): a link's byte sum passes 2^32."""
    pk = tie["pk"]
    w = RC.big_weights(len(pk["src"]))
    assert int(w.max()) == 0xFFFFFFFF and int(w.min()) == 0
    link, _, _ = RR.link_load_round(tie["g"], tie["nodes"], (0, 300), tie["pred"], tie["hosts"], pk, tie["status"], w)
    print(f"case (b): {int((link >= 1 << 32).sum())} links past 2^32, the largest {int(link.max())}")
    assert int((link >= 1 << 32).sum()) >= 1


def test_case_c_conditions():
    """(c): each of the four statuses at least 100 times."""
    st = RC.mixed_status(20000)
    cnt = np.bincount(st, minlength=4)
    print(f"case (c): statuses {cnt.tolist()}")
    assert len(cnt) == 4 and cnt.min() >= 100


def test_path_and_star_conditions(oracle):
    """(f): the path's deepest walked packet has 4,095 hops; the star's link from the sending
    spoke to the hub carries packets to at least 500 distinct destinations."""
    g = LC.path_graph(4096)
    nodes = np.arange(4096, dtype=np.uint32)
    hosts, pk = RC.path_round()
    assert len(pk["src"]) == 2000
    _, _, hops = RR.link_load_round(g, nodes, (0, 64), _trees(oracle, g, nodes, (0, 64)), hosts, pk)
    assert int(hops.max()) == 4095
    g = LC.star_graph(512)
    nodes = np.arange(513, dtype=np.uint32)
    pred = _trees(oracle, g, nodes, (0, 8))
    hosts, pk = RC.star_round()
    idx, ri, cj = RR.counted_pairs(hosts, pk, None)
    assert (ri == 1).all()
    through_hub = np.unique(cj[pred[1, cj] == 0])  # (one host per node: column = destination)
    through_hub = np.union1d(through_hub, cj[cj == 0])
    link, _, hops = RR.link_load_round(g, nodes, (0, 8), pred, hosts, pk)
    _, _, keys = LR.links(g)
    hub = int(LR.link_index(keys, [1], [0])[0])
    print(f"star: {len(np.unique(cj))} distinct destinations, {int(link[hub])} packets on the link 1 -> 0")
    assert len(through_hub) >= 500 and int(link[hub]) >= 500
    assert int(link[hub]) == int(np.isin(cj, through_hub).sum())


def test_other_inputs_qualify(oracle):
    """(d), (e), (i): senders on their row blocks, same-node batches, unknown addresses marked."""
    nodes, hosts, lo, hi = RC.shuffled_round()
    assert (hosts["route"] < 120).all()
    assert (hosts["route"][lo["src"]] < 60).all() and (hosts["route"][hi["src"]] >= 60).all()
    assert sorted(nodes.tolist()) == list(range(300)) and not np.array_equal(nodes, np.arange(300))
    for g in (LC.directed_graph(), LC.multi_graph()):
        hosts, pk = RC.same_node_round(g["n"])
        idx, ri, cj = RR.counted_pairs(hosts, pk, None)
        assert np.array_equal(ri, cj) and len(idx) == 2 * g["n"]
    hosts, pk, status = RC.sparse_address_round()
    assert int(hosts["ip"].max()) - int(hosts["ip"].min()) > 1 << 30  # no dense window
    assert 100 < int((status == RC.DROP_NO_DST).sum()) < 1000
    assert RR.first_bad_packet(hosts, pk, status, (0, 300), 300) is None
    assert RR.first_bad_packet(hosts, pk, None, (0, 300), 300) == int(np.flatnonzero(status)[0])


def test_symbol_exported():
    so = os.path.join(ROOT, "shadow_amd", "libshadow_gpu.so")
    assert os.path.exists(so), "libshadow_gpu.so is not built"
    if not shutil.which("nm"):
        pytest.skip("nm missing")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == "sg_link_load_packets" for ln in out.splitlines())
    from shadow_amd import _capi

    assert "sg_link_load_packets" in _capi.EXPORTED
