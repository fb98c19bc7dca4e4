"""The inputs of the group's link-trace cases (tests/group_trace_cases.py), qualified by the
references alone: the tie round split over 2, 3 and 8 members really has links and (link, enter)
groups that several members share, so the merge and its member tie-break decide an order; the
fan-in case really has the stated per-member segment lengths on the shared link.  No GPU."""
import numpy as np
import pytest

import group_trace_cases as GC
import link_cases as LC
import link_ref as LR
import trace_cases as XC
import trace_ref as XR
import tree_ref as R


def _table(O, g, nodes=None):
    nodes = np.arange(g["n"], dtype=np.uint32) if nodes is None else nodes
    rc, lat, loss, _ = O.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], nodes,
                                        rows=(0, g["n"]), threads=4)
    assert rc == 0
    pred, _, bad = R.tree_ref(g, nodes, (0, g["n"]), lat, loss)
    assert bad is None
    return nodes, lat, pred


@pytest.fixture(scope="module")
def tie(oracle):
    g = LC.tie_graph()
    nodes, lat, pred = _table(oracle, g)
    hosts, pk, mixed = XC.tie_round()
    return dict(g=g, nodes=nodes, lat=lat, pred=pred, hosts=hosts, pk=pk, mixed=mixed)


@pytest.mark.parametrize("world", GC.WORLDS)
def test_tie_round_split(tie, world):
    """Every member has packets; at least 500 links hold records of two or more members and at
    least 100 (link, enter_ns) groups do, under the mixed statuses and under none; the split
    loses nothing: the concatenated batch's trace has the whole batch's offsets."""
    g, nodes, hosts, pk = tie["g"], tie["nodes"], tie["hosts"], tie["pk"]
    whole = XR.trace(g, nodes, (0, 300), tie["pred"], tie["lat"], hosts, pk, tie["mixed"])
    for status in (tie["mixed"], None):
        parts = GC.split(hosts, pk, status, 300, world)
        assert len(parts) == world and all(len(p[2]) > 0 for p in parts)
        links, groups = GC.shared(g, nodes, 300, tie["pred"], tie["lat"], hosts, parts)
        print(f"W = {world}, status {'mixed' if status is not None else 'none'}: {links} links and {groups} "
              f"(link, enter) groups hold records of two or more members")
        assert links >= 500 and groups >= 100
    parts = GC.split(hosts, pk, tie["mixed"], 300, world)
    got = GC.trace(g, nodes, 300, tie["pred"], tie["lat"], hosts, parts)
    assert np.array_equal(got[0], whole[0]) and len(got[1]) == len(whole[1])
    # the member of a record is the owner of its packet's sender
    cat, _, bases = GC.concat(parts)
    row = hosts["route"][cat["src"][got[1]]].astype(np.int64)
    lo = np.array([b[0] for b in GC.blocks(300, world)])
    assert np.array_equal(got[2], (np.searchsorted(lo, row, side="right") - 1).astype(np.uint8))


@pytest.mark.parametrize("times", ["equal", "tied", "shuffled"])
def test_fan_in_lengths(oracle, times):
    """The last link of the path holds exactly lengths[m] records of member m; every length of
    FAN_LENGTHS occurs, 0 beside 2049; "tied": one enter time there, the order by member then
    packet; "shuffled": distinct enter times, the members interleaved."""
    g, nodes = GC.fan_graph(), GC.fan_nodes()
    _, lat, pred = _table(oracle, g, nodes)
    _, _, keys = LR.links(g)
    last = int(LR.link_index(keys, [GC.FAN_N - 2], [GC.FAN_N - 1])[0])
    assert sorted({k for c in GC.FAN_CASES for k in c}) == sorted(GC.FAN_LENGTHS)
    assert any(0 in c and 2049 in c for c in GC.FAN_CASES)
    assert [r1 - r0 for r0, r1 in GC.blocks(GC.FAN_N, GC.FAN_W)] == [2, 2, 2]
    for lengths in GC.FAN_CASES:
        hosts, parts = GC.fan_round(lengths, times)
        for m, (pk, _, _) in enumerate(parts):  # member m's packets are its own block's
            assert ((hosts["route"][pk["src"]] // 2) == m).all() and len(pk["src"]) == lengths[m]
        off, packet, member, hop, enter, _ = GC.trace(g, nodes, GC.FAN_N, pred, lat, hosts, parts)
        a, b = int(off[last]), int(off[last + 1])
        assert b - a == sum(lengths)
        assert np.bincount(member[a:b], minlength=GC.FAN_W).tolist() == list(lengths)
        if times == "tied":
            assert len(np.unique(enter[a:b])) == 1
            assert np.array_equal(member[a:b], np.sort(member[a:b])) and np.array_equal(packet[a:b], np.arange(b - a))
        elif times == "shuffled":
            assert len(np.unique(enter[a:b])) == b - a
            if sum(k > 1 for k in lengths) >= 2:
                assert not np.array_equal(member[a:b], np.sort(member[a:b]))
