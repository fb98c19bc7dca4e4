"""The inputs of the seam tests qualify by the references alone (tests/seam_cases.py): in every
case the oracle's table holds the cells S - 3 .. S + 2 (S = 2^32 - 1) exactly where the
construction puts them, the trees are tight, and the row block holds rows of both kinds."""
import numpy as np
import pytest

import seam_cases as SM
import sweep_cases as SC
import tree_ref as TR

S = SM.S
DIRECTED = [k for k, c in SM.CASES.items() if c[0] == "spur"]
UNDER = [k for k, c in SM.CASES.items() if c[0] == "under"]


def _table(oracle, name):
    """(case, build info, whole-table latency and loss by node index, the references per view)."""
    c, b, rs = SC.case(name), SM.build(name), SC.refs(oracle, name)
    n, nodes = c["g"]["n"], c["nodes"].astype(np.int64)
    assert rs[0]["rc"] == 0
    lat, loss = np.zeros((n, n), np.uint64), np.zeros((n, n), np.float32)
    lat[np.ix_(nodes, nodes)], loss[np.ix_(nodes, nodes)] = rs[0]["lat"], rs[0]["loss"]
    return c, b, lat, loss, rs


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def test_names():
    assert SM.CHAIN_ONLY == ("under_ms600", "under_unit600") and len(SM.SMALL) == 6
    assert set(SM.SMALL) <= set(SC.NAMES) and not set(SM.CHAIN_ONLY) & set(SC.NAMES)
    assert SC.NAMES[:SC.N_CASES] == [f"k{k:02d}" for k in range(SC.N_CASES)]


@pytest.mark.parametrize("name", list(SM.CASES))
def test_case_is_built_as_described(oracle, name):
    """Oracle rc 0 and a tight in-arc for every cell in both views; one self-loop of latency u per
    added node, no arc below u, dense exactly where meant; the generator's Bellman-Ford distances
    are the oracle's hub row."""
    c, b, lat, _, rs = _table(oracle, name)
    g, u, n0 = c["g"], b["u"], SM.CASES[name][1]
    for r in rs:
        assert r["rc"] == 0 and r["bad"] is None, (name, r["rc"], r.get("bad"))
    assert int(g["lat"].min()) == u
    loops = g["src"] == g["dst"]
    assert int(loops.sum()) == g["n"] and (g["lat"][loops & (g["src"] >= n0)] == u).all()
    assert SC.dense(g) == (name in SM.DENSE)
    off = np.arange(n0) != b["h"]
    assert np.array_equal(lat[b["h"], :n0][off], b["d0"][off].astype(np.uint64))
    assert g["directed"] == (b["kind"] == "spur")
    assert not np.array_equal(g["src"][-(g["n"] - n0):], np.arange(n0, g["n"]))  # shuffled


@pytest.mark.parametrize("name", DIRECTED)
def test_spur(oracle, name):
    c, b, lat, loss, _ = _table(oracle, name)
    n = c["g"]["n"]
    h, dn, f, g2, spur_loss = b["h"], b["dn"], b["f"], b["g2"], SM.CASES[name][6]
    off = ~np.eye(n, dtype=bool)
    rowmax = np.where(off, lat, 0).max(1)
    for e in SM.SPUR_OFFS:
        s = b["spurs"][e]
        assert int(lat[s, dn]) == S + e and int(rowmax[s]) == S + e, (name, e)
        # the loss at dn folds row s's cell of f through the 0.5 arc, not g2's through the decoy
        assert _bits(loss[s, dn]) == _bits(TR.fold(loss[s, f], np.float32(0.5)))
        assert _bits(loss[s, dn]) != _bits(TR.fold(loss[s, g2], np.float32(1.0)))
        assert _bits(loss[s, h]) == _bits(TR.fold(np.float32(0.0), np.float32(1) - np.float32(spur_loss)))
    for e in SM.ARC_OFFS:
        assert int(lat[b["arc_spurs"][e], h]) == S + e
    under = (rowmax >= S - 3) & (rowmax <= S - 1)
    assert int(under.sum()) == 3 and (rowmax == S - 1).any() and (rowmax == S - 2).any()
    wide = ((lat >= S) & off).any(1)
    assert int(wide.sum()) == 6 and not wide.all()
    assert ((lat == S) & off).any() and ((lat == S + 1) & off).any() and ((lat > 1 << 32) & off).any()
    assert n == SM.CASES[name][1] + 10


@pytest.mark.parametrize("name", UNDER)
def test_under(oracle, name):
    c, b, lat, _, _ = _table(oracle, name)
    n = c["g"]["n"]
    off = ~np.eye(n, dtype=bool)
    rowmax = np.where(off, lat, 0).max(1)
    at_seam = np.flatnonzero(rowmax == S - 1)
    assert len(at_seam) >= 20 and np.array_equal(at_seam, b["level"])
    wide = ((lat >= S) & off).any(1)
    assert int(wide.sum()) >= 3 and all(wide[s] for s in b["spurs"].values())
    assert int((rowmax < S - 1).sum()) >= 20
    assert not ((lat >= S) & (lat <= S + 2) & off).any()
    counts = [int(((lat == S + e) & off).sum()) for e in (-3, -2, -1)]
    assert counts == [2 * len(at_seam)] * 3, counts
    print(f"{name}: {len(at_seam)} of {n} rows with maximum S - 1, {int(wide.sum())} with a cell >= S, {counts[0]} cells each")


def test_across(oracle):
    c, b, lat, _, _ = _table(oracle, "across_ms129")
    n = c["g"]["n"]
    off = ~np.eye(n, dtype=bool)
    narrow = ((lat < S - 3) & off).any(1)
    for e in SM.SPUR_OFFS:
        rows = ((lat == S + e) & off).any(1)
        assert rows.any(), e
        if e >= 0:
            assert narrow[rows].all()
    assert len(b["level"]) >= 20
    for v in b["level"]:
        assert sorted(int(lat[v, s]) - S for s in b["spurs"].values()) == list(SM.SPUR_OFFS)


@pytest.mark.parametrize("name", list(SM.CASES))
def test_row_block(oracle, name):
    """The second view holds a row whose maximum is in [S - 3, S - 1] and a row with a cell >= S.
    ("across" has no row of the first kind, its level rows running on to S + 2: there the block
    holds a row with cells in [S - 3, S - 1] beside cells >= S.)"""
    c, r = SC.case(name), SC.refs(oracle, name)[1]
    r0, r1 = c["views"][1]["rows"]
    n = c["g"]["n"]
    assert 0 <= r0 < r1 <= n and r1 - r0 < n
    off = np.ones((r1 - r0, n), bool)
    off[np.arange(r1 - r0), np.arange(r0, r1)] = False
    lat = r["lat"]
    rowmax = np.where(off, lat, 0).max(1)
    wide = ((lat >= S) & off).any(1)
    assert wide.any() and not wide.all()
    if SM.CASES[name][0] == "across":
        assert (((lat >= S - 3) & (lat <= S - 1) & off).any(1) & wide).any()
    else:
        assert ((rowmax >= S - 3) & (rowmax <= S - 1)).any()
