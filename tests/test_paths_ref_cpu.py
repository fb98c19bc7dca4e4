"""The batched tree-path reference (tests/paths_ref.py) on a hand graph with every record
written out, its conservation law against the per-packet link-load reference, and the conditions
the GPU cases' inputs must meet (test_paths_gpu.py), checked here so that the inputs qualify by
the references alone.  The built library must export the two new entry points.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import link_cases as LC
import link_ref as LR
import link_round_cases as RC
import link_round_ref as RR
import paths_cases as PC
import paths_ref as PR
import tree_ref as R
from shadow_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    """A tree plus one chord and a parallel pair, 1 us arcs except the chord; the arcs 0 - 2 and
    2 - 5 lose half their packets (exact in f32), the others none:
           0 - 1 - 3        1 = 1 (two edges)     4 - 5 costs 9 us (never on a shortest path)
           |   |
           2   4            2 - 5
    """
    edges = [(0, 1, 1, 0.0), (0, 1, 1, 0.0), (0, 2, 1, 0.5), (1, 3, 1, 0.0), (1, 4, 1, 0.0), (2, 5, 1, 0.5),
             (4, 5, 9, 0.0)]
    src = list(range(6)) + [e[0] for e in edges]
    dst = list(range(6)) + [e[1] for e in edges]
    lat = [1000] * 6 + [1000 * e[2] for e in edges]
    loss = [0.0] * 6 + [e[3] for e in edges]
    return dict(n=6, src=np.uint32(src), dst=np.uint32(dst), lat=np.uint64(lat), loss=np.float32(loss), directed=False)


def test_hand_graph(oracle):
    g = _hand_graph()
    _, _, keys = LR.links(g)
    nodes, rows, lat, loss, pred = _table(oracle, g)
    assert pred[0].tolist() == [0, 0, 0, 1, 1, 2]
    k = lambda u, v: int(LR.link_index(keys, [u], [v])[0])
    # pairs: 0 - 1 - 3, 0 - 2 - 5, the self-loop of node 0, 3 - 1 - 0 - 2 - 5, one that does not count, 0 - 1
    ri, cj = np.int64([0, 0, 0, 3, -1, 0]), np.int64([3, 5, 0, 5, -1, 1])
    off, node, link, rl, rf = PR.records(g, nodes, rows, pred, lat, loss, ri, cj)
    assert off.tolist() == [0, 2, 4, 5, 9, 9, 10] and off.dtype == np.uint64
    assert node.tolist() == [1, 3, 2, 5, 0, 1, 0, 2, 5, 1]
    assert link.tolist() == [k(0, 1), k(1, 3), k(0, 2), k(2, 5), k(0, 0), k(3, 1), k(1, 0), k(0, 2), k(2, 5), k(0, 1)]
    assert rl.tolist() == [1000, 2000, 1000, 2000, 1000, 1000, 2000, 3000, 4000, 1000]
    assert rf.tolist() == [0.0, 0.0, 0.5, 0.75, 0.0, 0.0, 0.0, 0.5, 0.75, 0.0]
    assert node.dtype == link.dtype == np.uint32 and rl.dtype == np.uint64 and rf.dtype == np.float32
    # the same pairs from packets: host h on node h, host 6 on node 0; packet 4 is dropped
    hosts = synth.make_hosts(7, 6)
    sends = [(0, 3, 0), (0, 5, 0), (0, 6, 0), (3, 5, 0), (0, 3, 1), (0, 1, 0)]
    pk = dict(src=np.uint32([s for s, _, _ in sends]), dst_ip=hosts["ip"][[d for _, d, _ in sends]])
    status = np.uint8([st for _, _, st in sends])
    got = PR.packet_records(g, nodes, rows, pred, lat, loss, hosts, pk, status)
    for a, b in zip(got, (off, node, link, rl, rf)):
        assert np.array_equal(a, b)
    assert PR.packet_records(g, nodes, rows, pred, lat, loss, hosts, pk, None)[0].tolist() == [0, 2, 4, 5, 9, 11, 12]
    # record counts = the per-packet link loads' hops
    _, _, hops = RR.link_load_round(g, nodes, rows, pred, hosts, pk, status)
    assert np.array_equal(np.diff(off.astype(np.int64)), np.where(hops == RC.UMAX, 0, hops))
    # what a bad input reports
    assert PR.first_bad_pair((0, 6), 6, [0, 5, 2], [5, 0, 3]) is None
    assert PR.first_bad_pair((0, 3), 6, [0, 5, 2], [5, 0, 6]) == 1
    assert PR.first_bad_pair((0, 6), 6, [0, 5, 2], [5, 0, 6]) == 2
    keep = ri >= 0
    assert PR.first_bad_pred(g, nodes, rows, pred, ri[keep], cj[keep]) is None
    p = pred.copy()
    p[3, 2] = 4  # (4, 2) is not a link: row 3's walk from node 5 crosses it at node 2
    assert PR.first_bad_pred(g, nodes, rows, p, ri, cj) == (3, 2)
    assert PR.first_bad_pred(g, nodes, rows, p, ri, cj, links=False) is None
    p[0, 3] = 99  # a value out of range is found while counting: ahead of any pair that is not a link
    assert PR.first_bad_pred(g, nodes, rows, p, ri, cj) == (0, 3)
    p = pred.copy()
    p[3, 0], p[3, 1] = 1, 0  # a 2-cycle under row 3's walk from node 5: its destination column
    assert PR.first_bad_pred(g, nodes, rows, p, ri, cj) == (3, 5)
    p[3, 2] = 4  # the non-link below the cycle does not come ahead of it
    assert PR.first_bad_pred(g, nodes, rows, p, ri, cj) == (3, 5)
    p = pred.copy()
    p[0, 4] = 99  # no pair crosses node 4
    assert PR.first_bad_pred(g, nodes, rows, p, ri, cj) is None


@pytest.fixture(scope="module")
def tie(oracle):
    g = LC.tie_graph()
    nodes, rows, lat, loss, pred = _table(oracle, g)
    hosts, pk = RC.tie_round()
    # the round's statuses, from the oracle's delivery round on the hosts' own streams
    rng = np.stack([oracle.xoshiro_seed(int(s)) for s in hosts["seed"]])
    ctr = np.zeros(hosts["n"], np.uint64)
    out = oracle.deliver_round(RC.ROUND_END, 2**63, 0, pk["src"], pk["dst_ip"], pk["payload"], pk["send_time"],
                               hosts["ip"], hosts["route"], lat, loss, rng, ctr)
    return dict(g=g, nodes=nodes, lat=lat, loss=loss, pred=pred, hosts=hosts, pk=pk, status=out["status"])


def test_conservation(tie):
    """One per record, added at the record's link, is the per-packet link load of the same batch;
    with the payload per record, its byte load; the records' nodes give the node load."""
    g, pk, nodes = tie["g"], tie["pk"], tie["nodes"]
    tail, head, _ = LR.links(g)
    for status in (tie["status"], None, RC.mixed_status(len(pk["src"]))):
        off, node, link, _, _ = PR.packet_records(g, nodes, (0, 300), tie["pred"], tie["lat"], tie["loss"], tie["hosts"],
                                                  pk, status)
        want_l, want_n, hops = RR.link_load_round(g, nodes, (0, 300), tie["pred"], tie["hosts"], pk, status)
        got = np.zeros(len(tail), np.uint64)
        np.add.at(got, link, np.uint64(1))
        assert np.array_equal(got, want_l)
        cnt = np.diff(off.astype(np.int64))
        assert np.array_equal(cnt, np.where(hops == RC.UMAX, 0, hops))
        want_b, _, _ = RR.link_load_round(g, nodes, (0, 300), tie["pred"], tie["hosts"], pk, status, pk["payload"])
        got = np.zeros(len(tail), np.uint64)
        np.add.at(got, link, np.repeat(pk["payload"].astype(np.uint64), cnt))
        assert np.array_equal(got, want_b)
        got = np.zeros(300, np.uint64)
        np.add.at(got, node[tail[link] != head[link]], np.uint64(1))
        assert np.array_equal(got, want_n)
        assert np.array_equal(head[link], node)


def test_case_conditions(tie, oracle):
    """(a): measured 12,377 of 20,000 packets counted, 36 of them same-node pairs, 49,989 records,
    the longest path 10 hops.  (b): the first wave's span and the capacities around it.  (f): the
    path's deepest packet has 4,095 records, more than any staging capacity."""
    g, pk, nodes = tie["g"], tie["pk"], tie["nodes"]
    ri, cj = PR.packet_pairs(tie["hosts"], pk, tie["status"])
    off = PR.records(g, nodes, (0, 300), tie["pred"], tie["lat"], tie["loss"], ri, cj)[0]
    cnt = np.diff(off.astype(np.int64))
    counted, same = int((ri >= 0).sum()), int(((ri >= 0) & (ri == cj)).sum())
    print(f"case (a): {counted} of {len(ri)} counted, {same} same-node, {int(off[-1])} records, longest {int(cnt.max())}")
    assert 0.3 * len(ri) < counted < 0.9 * len(ri) and same >= 10 and int(cnt.max()) >= 6
    assert ((cnt == 0) == (ri < 0)).all()
    for n_pairs in PC.PAIR_COUNTS:
        ri, cj = PC.tie_pairs(n_pairs)
        assert ri[0] == cj[0]
        off = PR.records(g, nodes, (0, 300), tie["pred"], tie["lat"], tie["loss"], ri.astype(np.int64), cj)[0]
        spans = PC.wave_spans(off)
        caps = PC.stage_capacities(off)
        assert len(spans) == (n_pairs + 63) // 64 and int(spans.sum()) == int(off[-1])
        print(f"case (b): {n_pairs} pairs, wave spans {spans.tolist()}, capacities {caps}")
        if n_pairs > 1:
            assert len(caps) == 3 and caps[0] - 1 == int(spans[0]) == caps[1] == caps[2] + 1
        if n_pairs == 257:  # at the middle capacity other waves lie on either side
            assert (spans > caps[1]).any() and (spans <= caps[1]).sum() >= 2
    gp = LC.path_graph(4096)
    nodes, rows, lat, loss, pred = _table(oracle, gp, rows=(0, 64))
    hosts, pk = RC.path_round()
    off = PR.packet_records(gp, nodes, rows, pred, lat, loss, hosts, pk)[0]
    assert int(np.diff(off.astype(np.int64)).max()) == 4095 and int(PC.wave_spans(off).min()) > 1536


def test_symbols_exported():
    so = os.path.join(ROOT, "shadow_amd", "libshadow_gpu.so")
    assert os.path.exists(so), "libshadow_gpu.so is not built"
    if not shutil.which("nm"):
        pytest.skip("nm missing")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    from shadow_amd import _capi

    for sym in ("sg_tree_paths", "sg_tree_paths_packets"):
        assert sym in names and sym in _capi.EXPORTED
