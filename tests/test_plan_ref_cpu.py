"""The CPU model of the phase plan (plan_ref.py) on hand-worked graphs, and the properties of the
plans of test_sssp_plan_gpu.py's graphs that those tests rely on (so a changed generator cannot
hollow them out)."""
import numpy as np

import plan_cases as C
import plan_ref as P

GRID = 256  # persistent workgroups of the LDS search on an MI355X: a phase with more rows can chain


def _graph(n, edges, directed=False):
    src, dst = np.array(edges, dtype=np.uint32).reshape(-1, 2).T
    return dict(n=n, src=src, dst=dst, directed=directed)


def _phases(g, n_phase, n_land=0, used=None, rows=None):
    used = np.arange(g["n"]) if used is None else used
    return list(P.phases(g, used, rows or (0, len(used)), n_phase, n_land))


def test_arcs_as_uploaded():
    """A self-loop is no arc; an undirected edge is an arc each way; parallel edges stay."""
    g = _graph(3, [(0, 0), (0, 1), (0, 1), (1, 2)])
    s, d = P.arcs(g)
    assert sorted(zip(s, d)) == [(0, 1), (0, 1), (1, 0), (1, 0), (1, 2), (2, 1)]
    g["directed"] = True
    s, d = P.arcs(g)
    assert sorted(zip(s, d)) == [(0, 1), (0, 1), (1, 2)]


def test_star():
    """Set 0: the hub's gain is 600, a leaf's 2, so every row names the hub.  Set 1: every leaf's
    gain is 1 and its only open candidate is itself.  Nothing is left for the later sets."""
    g = C.star()
    ph = P.phases(g, np.arange(600), (0, 600), 6)
    assert P.sizes(ph, 6) == [1, 599, 0, 0, 0, 0]
    assert ph[0] == 0
    assert P.sizes(P.phases(g, np.arange(600), (0, 600), 2), 2) == [1, 599]
    assert C.out_degrees(g)[0] == 599


def test_two_triangles():
    """Triangles 0-1-2 and 3-4-5 joined by 2-3.  Gains 3,3,4,4,3,3: rows 0-3 name 2 (3 sees the tie
    of 2 and itself: the lowest row), 4 and 5 name 3.  Set 1 (rows 0,1,4,5 open, gains 2 each): 0
    and 1 name 0, 4 and 5 name 4."""
    g = _graph(6, [(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 3), (2, 3)])
    assert _phases(g, 2) == [1, 1, 0, 0, 1, 1]
    assert _phases(g, 3) == [1, 2, 0, 0, 1, 2]
    # with a set 2, rows 1 and 5 (no open neighbour left) name themselves: phase 2 by vote, none left over
    assert _phases(g, 4) == [1, 2, 0, 0, 1, 2]
    assert P.sizes(P.phases(g, np.arange(6), (0, 6), 6), 6) == [2, 2, 2, 0, 0, 0]


def test_parallel_arcs_count():
    """Row 0 sees 1 (neighbours 0, 3, 4) and 2 (neighbour 0 and a triple edge to 5).  With arcs
    counted 2's gain is 5 against 4 and 0 names 2; with neighbours counted it would be 3 against 4."""
    g = _graph(6, [(0, 1), (0, 2), (1, 3), (1, 4), (2, 5), (2, 5), (2, 5)])
    assert _phases(g, 2) == [1, 0, 0, 1, 1, 1]


def test_directed_three_cycle():
    """0 -> 1 -> 2 -> 0, every gain 2: 0 names 0 (lowest of 0, 1), 1 names 1, 2 names 0.  In set 1
    row 2 is alone and names itself."""
    g = _graph(3, [(0, 1), (1, 2), (2, 0)], directed=True)
    assert _phases(g, 2) == [0, 0, 1]
    assert _phases(g, 3) == [0, 0, 1]
    assert P.sizes(P.phases(g, np.arange(3), (0, 3), 3), 3) == [2, 1, 0]


def test_blocks_and_subsets_see_block_rows_only():
    """Path 0-1-2-3-4.  All rows: gains 2,3,3,3,2, rows 0,1,2 name 1, 3 names 2, 4 names 3.  The
    block of rows 2..4: 2-3-4 is a path of its own, every row names 3.  Used (4, 2, 0): no arcs
    inside, every row names itself."""
    g = _graph(5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    assert _phases(g, 2) == [1, 0, 0, 0, 1]
    assert _phases(g, 2, rows=(2, 5)) == [1, 0, 1]
    assert _phases(g, 2, used=np.array([4, 2, 0])) == [0, 0, 0]
    assert _phases(g, 2, used=np.array([3, 0, 4, 1]), rows=(0, 3)) == [0, 0, 1]


def test_landmarks_relabel():
    """Ten disjoint edges (2i, 2i+1): phase 0 is the ten even rows.  Index i of them is a landmark
    where floor(i * n_land / 10) steps, and i = 0: with 4 landmarks i = 0, 3, 5, 8."""
    g = _graph(20, [(2 * i, 2 * i + 1) for i in range(10)])
    assert _phases(g, 2) == [0, 1] * 10
    ph = _phases(g, 2, 4)
    assert [r for r in range(20) if ph[r] == 0] == [0, 6, 10, 16]
    assert [ph[r] for r in range(1, 20, 2)] == [2] * 10
    assert sorted(set(ph[r] for r in range(0, 20, 2))) == [0, 1]
    # n_land >= |phase 0|: no landmark, every phase one later
    assert _phases(g, 2, 10) == [1, 2] * 10
    assert _phases(g, 2, 9).count(0) == 9


def test_launch_counts():
    assert [P.n_launches(k) for k in (1, 2, 3, 6, 9)] == [2, 2, 3, 6, 6]
    assert [P.n_launches(k, 8) for k in (2, 5, 6)] == [3, 6, 6]


def test_big_graph_phases_can_chain():
    g, used = C.big(), np.arange(2400)
    s3 = P.sizes(P.phases(g, used, (0, 2400), 3), 3)
    s4 = P.sizes(P.phases(g, used, (0, 2400), 4), 4)
    s6 = P.sizes(P.phases(g, used, (0, 2400), 6), 6)
    assert s3 == [650, 696, 1054] and s4 == [650, 696, 627, 427]
    assert min(s3) > GRID and min(s4) > GRID
    assert sum(s6) == 2400 and 0 in s6


def test_small_graph_phases_below_the_grid():
    s6 = P.sizes(P.phases(C.small(), np.arange(900), (0, 900), 6), 6)
    assert s6 == [239, 260, 223, 163, 15, 0]
    assert any(0 < s < GRID for s in s6)


def test_blocks_and_subset_of_the_big_graph():
    g = C.big()
    assert len(C.SUBSET) % 4 != 0 and len(np.unique(C.SUBSET)) == 1801
    assert not np.array_equal(C.SUBSET, np.sort(C.SUBSET))
    for used, rows in ((np.arange(2400), (600, 1900)), (C.SUBSET, (0, 1801)), (C.SUBSET, (300, 1500))):
        s4 = P.sizes(P.phases(g, used, rows, 4), 4)
        assert sum(s4) == rows[1] - rows[0] and all(s4), s4
        assert s4[1] > GRID  # the first bounded launch can chain


def test_landmark_cases():
    g, used = C.big(), np.arange(2400)
    for n_land in (8, 64):
        for n_phase in (2, 5, 6):
            n = P.n_launches(n_phase, n_land)
            s = P.sizes(P.phases(g, used, (0, 2400), n_phase, n_land), n)
            assert s[0] == n_land and s[0] + s[1] == 650 and sum(s) == 2400
            assert s[1] > GRID  # the landmark-bounded launch can chain
    for sub, rows in ((used, (600, 1900)), (C.SUBSET, (0, 1801)), (C.SUBSET, (300, 1500))):
        s = P.sizes(P.phases(g, sub, rows, 3, 16), 4)
        assert s[0] == 16 and s[1] > GRID and sum(s) == rows[1] - rows[0]
    assert P.sizes(P.phases(g, used, (0, 2400), 2, 100000), 3) == [0, 650, 1750]
    assert P.sizes(P.phases(C.star(), np.arange(600), (0, 600), 2, 8), 3) == [0, 1, 599]
    s = P.sizes(P.phases(C.far(), np.arange(620), (0, 620), 2, 8), 3)
    assert s[0] == 8 and s[1] > 0


def test_hub_degrees():
    """Out-degrees on both sides of 8 and of 64; a leaf of the star sees 599 arcs two hops out."""
    d = C.out_degrees(C.hubs())
    assert d.min() < 8 and ((d > 8) & (d <= 20)).sum() > 100 and ((d > 20) & (d < 64)).any() and d.max() > 64
    assert d[0] >= 150 and d[400] >= 40
    z = C.hubs(zero=1.0)
    assert not z["loss"].any() and np.array_equal(z["src"], C.hubs()["src"])
    assert not C.star(zero=1.0)["loss"].any()
