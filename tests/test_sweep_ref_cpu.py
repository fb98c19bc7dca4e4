"""The inputs of test_sweep_gpu.py qualify by the references alone (tests/sweep_cases.py): every
generated case builds in the oracle and has a tree, the family covers what it is meant to cover,
the disconnected graphs succeed and fail as the oracle says, and the vectorised walk that checks
the scan's second trip agrees with tests/paths_ref.py."""
import numpy as np
import pytest

import paths_cases as PC
import paths_ref as PR
import sweep_cases as SC
import tree_cases as TC
import tree_ref as TR

GENERATED = SC.NAMES[:SC.N_CASES]


def _off_diagonal(n, rows):
    r0, r1 = rows
    off = np.ones((r1 - r0, n), bool)
    off[np.arange(r1 - r0), np.arange(r0, r1)] = False
    return off


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_qualifies(oracle, name):
    """rc 0 from the oracle, a tight in-arc for every cell, and 200 sampled tree paths per view
    that refold to the table's bits."""
    c = SC.case(name)
    g, nodes = c["g"], c["nodes"]
    n = g["n"]
    assert sorted(nodes.tolist()) == list(range(n))
    assert int((g["src"] == g["dst"]).sum()) == n  # one self-loop per node
    idx = TR.build_arc_index(g)
    for v, r in zip(c["views"], SC.refs(oracle, name)):
        r0, r1 = v["rows"]
        assert r["rc"] == 0, (name, r["rc"], r["first"])
        assert r["bad"] is None, (name, r["bad"])
        rng = np.random.default_rng(5)
        for i, j in zip(rng.integers(0, r1 - r0, SC.SAMPLE).tolist(), rng.integers(0, n, SC.SAMPLE).tolist()):
            s, d = int(nodes[r0 + i]), int(nodes[j])
            if s == d:
                continue
            path = TR.expand(r["pred"][i], nodes, s, d)
            assert path[1] == r["hop"][i, j]
            wl, wf = np.zeros(n, np.uint64), np.zeros(n, np.float32)
            wl[nodes], wf[nodes] = r["lat"][i], r["loss"][i]
            l2, f2 = TR.refold(g, path, wl, wf, idx)
            assert l2 == int(r["lat"][i, j]) and np.float32(f2).view(np.uint32) == r["loss"][i, j].view(np.uint32)
        # the batches: senders inside the block, pairs inside it, same-node pairs among them
        ri, cj = v["pairs"]
        assert len(ri) == SC.N_PAIRS and ((ri >= r0) & (ri < r1)).all() and (cj < n).all() and (ri == cj).any()
        assert ((c["hosts"]["route"][v["pk"]["src"]] >= r0) & (c["hosts"]["route"][v["pk"]["src"]] < r1)).all()
        assert len(v["pk"]["src"]) == min(4000, 40 * n) and len(set(v["status"].tolist())) > 1
        assert v["counts"].shape == (r1 - r0, n) and int(v["counts"].max()) < 1 << 40
        assert int(np.diff(r["records"][0].astype(np.int64)).min()) >= 1


def test_family_covers(oracle):
    """The counts the family is built for."""
    ax = [SC.case(k)["axes"] for k in GENERATED]
    assert len(ax) == 40
    big = [a for a in ax if a[0] >= 63]
    assert {a[1] for a in big} == {False, True}
    assert {a[3] for a in big} == set(SC.LAT_REGIMES) and {a[4] for a in big} == set(SC.LOSS_REGIMES)
    assert {1, 2, 3} <= {a[0] for a in ax} and {a[0] for a in ax} == set(SC.NODE_COUNTS)
    assert {a[2] for a in ax} == set(SC.DEGREES)
    tied, wide, mixed, mixed_block = [], [], [], []
    for k in GENERATED:
        c, r = SC.case(k), SC.refs(oracle, k)[0]
        n = c["g"]["n"]
        off = _off_diagonal(n, (0, n))
        if (r["tight"][off] > 1).any():
            tied.append(k)
        w = ((r["lat"] >= SC.WIDE_NS) & off).any(1)
        if w.any():
            wide.append(k)
        if w.any() and not w.all():
            mixed.append(k)
            # ... in the row block too, where the case has one
            v1 = SC.refs(oracle, k)[1]
            w1 = ((v1["lat"] >= SC.WIDE_NS) & _off_diagonal(n, c["views"][1]["rows"])).any(1)
            if w1.any() and not w1.all():
                mixed_block.append(k)
    assert len(tied) >= 12, tied
    assert len(mixed_block) >= 1
    assert len(wide) >= 4, wide
    # rows with a wide cell beside rows without any: k_tree_lds sends the former to the global
    # path one by one while their neighbours stay in LDS
    assert len(mixed) >= 1 and {"k18", "k28"} <= set(mixed), mixed
    # the outliers are avoided by every shortest path: only the 1-3 s regime gives wide cells
    assert {SC.case(k)["axes"][3] for k in wide} == {"wide"}
    assert not any(SC.dense(SC.case(k)["g"]) for k in GENERATED)
    # SG_PATHS_STAGE_HOPS=64: cases where some waves' spans fit the staging capacity and others do not
    split_pairs, split_packets = [], []
    for k in GENERATED:
        c, v, r = SC.case(k), SC.case(k)["views"][0], SC.refs(oracle, k)[0]
        spans = PC.wave_spans(r["records"][0])
        if (spans <= 64).any() and (spans > 64).any():
            split_pairs.append(k)
        off = PR.packet_records(c["g"], c["nodes"], v["rows"], r["pred"], r["lat"], r["loss"], c["hosts"], v["pk"], v["status"])[0]
        spans = PC.wave_spans(off)
        if (spans <= 64).any() and (spans > 64).any():
            split_packets.append(k)
    assert len(split_pairs) >= 1 and len(split_packets) >= 4, (split_pairs, split_packets)


def test_split_graphs(oracle):
    """The oracle's answer for each graph that is not one strongly connected piece: rc 0 where
    every used pair is connected, ERR_UNREACHABLE otherwise, its first pair's row inside the
    block used."""
    for name, (g, used, rows) in SC.split_cases().items():
        rc, _, _, _ = SC.oracle_rows(oracle, g, used, rows)
        assert rc == 0, (name, rc)
    firsts = {}
    for name, (g, used, rows) in SC.error_cases().items():
        rc, _, _, first = SC.oracle_rows(oracle, g, used, rows)
        assert rc == oracle.ERR_UNREACHABLE, (name, rc)
        r0, r1 = rows or (0, len(used))
        assert r0 <= first[0] < r1 and first[1] < len(used), (name, first)
        firsts[name] = first
        # the valid build that follows it: a used list of the other kind
        g2, used2 = SC.follow_up(name)
        assert SC.oracle_rows(oracle, g2 or g, used2)[0] == 0, name
        ident = lambda u: np.array_equal(u, np.arange(len(u)))
        assert ident(used) != ident(used2), name
    assert firsts["E1"] == (0, 6) and firsts["E1_rows"] == (100, 6)
    assert firsts["E2_identity"] == (600, 0) and firsts["E2_shuffled"] == (1, 0)
    # the isolated nodes have no self-loop and D is dense by the library's rule
    und = SC.islands(False)
    assert und["n"] == 703 and int(max(und["src"].max(), und["dst"].max())) == 699
    assert SC.dense(SC.dense_blocks()) and not SC.dense(SC.islands(True))


def test_walk_is_paths_ref(oracle):
    """The vectorised walk of the scan test against paths_ref.records on a 2,000-pair sample of
    its own batch, the last pair included."""
    g = TC.multi_graph()
    nodes = np.arange(64, dtype=np.uint32)
    rc, lat, loss, _ = SC.oracle_rows(oracle, g, nodes)
    assert rc == 0
    pred, _, bad = TR.tree_ref(g, nodes, (0, 64), lat, loss)
    assert bad is None
    assert SC.SCAN_PAIRS == 1024 * 2048 + 1
    ri, cj = SC.scan_pairs(64)
    assert len(ri) == SC.SCAN_PAIRS and ri[-1] == cj[-1]
    pick = np.concatenate([np.random.default_rng(3).integers(0, SC.SCAN_PAIRS, 1999), [SC.SCAN_PAIRS - 1]])
    off, node, link = SC.walk_records(g, nodes, (0, 64), pred, ri[pick], cj[pick])
    want = PR.records(g, nodes, (0, 64), pred, lat, loss, ri[pick].astype(np.int64), cj[pick])
    assert np.array_equal(off, want[0]) and np.array_equal(node, want[1]) and np.array_equal(link, want[2])
    assert int(off[-1]) - int(off[-2]) == 1
