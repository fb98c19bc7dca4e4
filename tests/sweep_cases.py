"""A generated family of graphs carried through every routing stage, table to hop records
(test_sweep_ref_cpu.py qualifies them on the CPU, test_sweep_gpu.py runs them), the disconnected
graphs of the table builds, and the batch that takes the hop-record scan into its second trip.

Case k of CASES takes each axis from a list by an index that is a function of k alone; the
indices are chosen so that the axes do not move in step (the node counts have period 12, the
latency regimes 5, and the other three shift by one with every cycle of the node counts).
Every random draw comes from default_rng(SEED0 + k): a case never changes with its neighbours.
Beside the 40, EXTRA pins the seam cases of tests/seam_cases.py by name.
"""
import functools

import numpy as np

from shadow_amd import synth

import link_ref as LR
import link_round_cases as RC
import link_round_ref as RR
import paths_ref as PR
import tree_ref as TR

WIDE_NS = 1 << 32
SEED0 = 7000
N_CASES = 40
NODE_COUNTS = (1, 2, 3, 5, 17, 63, 64, 65, 129, 200, 257, 300)
DEGREES = (2.0, 3.0, 6.0, 12.0)
LAT_REGIMES = ("unit", "ms", "us", "wide", "outliers")
LOSS_REGIMES = ("zero", "half", "four", "uniform", "tie", "one")
N_PAIRS = 2000
SAMPLE = 200


def axes(k):
    """(n, directed, mean degree, latency regime, loss regime) of case k."""
    c = k // len(NODE_COUNTS)
    return (NODE_COUNTS[k % len(NODE_COUNTS)], bool((k // 3 + c) % 2), DEGREES[(k + c) % len(DEGREES)],
            LAT_REGIMES[k % len(LAT_REGIMES)], LOSS_REGIMES[(k + 2 * c) % len(LOSS_REGIMES)])


def _latencies(rng, regime, m):
    if regime == "unit":  # every arc 1 us
        return np.full(m, 1000, np.uint64)
    if regime == "ms":  # {1..4} ms: many equal-latency routes
        return rng.integers(1, 5, m).astype(np.uint64) * 1_000_000
    if regime == "us":  # 1-100 ms in us steps
        return rng.integers(1000, 100_001, m).astype(np.uint64) * 1000
    if regime == "wide":  # 1-3 s: paths run past 2^32 ns
        return rng.integers(1_000_000, 3_000_001, m).astype(np.uint64) * 1000
    lat = rng.integers(1, 5, m).astype(np.uint64) * 1_000_000  # "outliers": 5 % of the arcs 3 s
    lat[rng.random(m) < 0.05] = np.uint64(3_000_000_000)
    return lat


def _losses(rng, regime, m):
    if regime == "zero":
        return np.zeros(m, np.float32)
    if regime == "half":  # folds are exact
        return np.where(rng.random(m) < 0.5, 0.5, 0.0).astype(np.float32)
    if regime == "four":  # tree_cases.suffix_graph's values: folds differ with the order of the factors
        return rng.choice(np.array([0.05, 0.1, 0.2, 0.3], np.float32), m)
    loss = rng.uniform(0.0, 0.02, m).astype(np.float32)
    if regime == "tie":  # tree_cases.tie_graph's mix
        loss[rng.random(m) < 0.9] = 0.5
        loss[rng.random(m) < 0.6] = 0.0
    elif regime == "one":  # 10 % of the arcs lose every packet
        loss[rng.random(m) < 0.1] = 1.0
    return loss


def graph(n, directed, degree, lat_regime, loss_regime, seed):
    """One self-loop per node, a ring (both ways when directed), random chords to the mean
    degree, 15 % of the non-loop edges once more as parallel edges with weights of their own,
    the edge order shuffled."""
    rng = np.random.default_rng(seed)
    ring = np.arange(n)
    s, d = [ring], [ring]
    if n > 1:
        s.append(ring)
        d.append((ring + 1) % n)
        if directed:
            s.append((ring + 1) % n)
            d.append(ring)
    m = max(0, int(n * degree / (1 if directed else 2)) - n)
    cs, cd = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = cs != cd
    src, dst = np.concatenate(s + [cs[keep]]), np.concatenate(d + [cd[keep]])
    other = np.flatnonzero(src != dst)
    dup = other[rng.random(len(other)) < 0.15]
    src, dst = np.concatenate([src, src[dup]]), np.concatenate([dst, dst[dup]])
    m = len(src)
    lat, loss = _latencies(rng, lat_regime, m), _losses(rng, loss_regime, m)
    p = rng.permutation(m)
    return dict(n=n, src=src[p].astype(np.uint32), dst=dst[p].astype(np.uint32), lat=lat[p], loss=loss[p],
                directed=directed)


def _round(hosts, n_packets, seed, src_hosts=None):
    pk = RC.batch(n_packets, hosts, seed, src_hosts=src_hosts)
    return pk, RC.mixed_status(n_packets, seed + 1)


def _make(name, n, directed, degree, lat_regime, loss_regime, seed, g=None, block=None):
    """With a ready graph `g` (built on graph()'s with these arguments) n is the graph's own;
    `block(nodes)` then gives the second view's rows in place of [n // 3, n - n // 4)."""
    if g is None:
        g = graph(n, directed, degree, lat_regime, loss_regime, seed)
    n = g["n"]
    rng = np.random.default_rng(seed + 100_000)
    nodes = rng.permutation(n).astype(np.uint32)
    blocks = [(0, n)] + ([block(nodes) if block else (n // 3, n - n // 4)] if n >= 3 else [])
    hosts = synth.make_hosts(3 * n, n)
    n_packets = min(4000, 40 * n)
    counts = np.where(rng.random((n, n)) < 0.3, rng.integers(1, 1 << 40, (n, n)), 0).astype(np.uint64)
    ri, cj = rng.integers(0, n, N_PAIRS), rng.integers(0, n, N_PAIRS)
    cj[:8] = ri[:8]  # same-node pairs, whatever n
    views = []
    for r0, r1 in blocks:
        senders = np.flatnonzero((hosts["route"] >= r0) & (hosts["route"] < r1))
        pk, status = _round(hosts, n_packets, seed + 200_000 + r0, src_hosts=senders)
        views.append(dict(rows=(r0, r1), pk=pk, status=status, counts=counts[r0:r1],
                          pairs=((r0 + ri % (r1 - r0)).astype(np.uint32), cj.astype(np.uint32))))
    return dict(name=name, g=g, nodes=nodes, hosts=hosts, views=views,
                axes=(n, directed, degree, lat_regime, loss_regime))


def _seam_args(name):
    """_make's arguments for a case of tests/seam_cases.py (which builds on graph() above and is
    therefore imported only when a case is made)."""
    import seam_cases

    return seam_cases.make_args(name)


# Cases pinned by name beside the 40: name -> a call that gives _make's arguments after the name.
# (Rows with a wide cell beside rows without any, where k_tree_lds sends single rows to the global
# path, needed no pin: k18 and k28 are such cases, as test_sweep_ref_cpu.py asserts.)  A case that
# exposed a bug stays here under its case number and stage.
#
# The seam cases: optima of exactly 2^32 - 4 .. 2^32 + 1 ns, where the searches' 32-bit keys
# saturate; two of them dense.  These names are the only list of them; seam_cases.CASES holds
# their parameters, and those of the two 603-node cases that case() makes for the chained-row
# tests alone.
SEAM = ("spur_us63", "spur_us200_lossy", "spur_dense", "under_ms129", "across_ms129", "under_dense")
EXTRA = {name: functools.partial(_seam_args, name) for name in SEAM}
NAMES = [f"k{k:02d}" for k in range(N_CASES)] + list(EXTRA)


@functools.lru_cache(maxsize=None)
def case(name):
    """Case `name` ("k00" .. "k39" or a key of EXTRA): the graph, `nodes` (a seeded permutation
    of every node), 3 n hosts, and per row block (the whole table; [n // 3, n - n // 4) when
    n >= 3) a round of min(4000, 40 n) packets from the block's hosts with mixed statuses, the
    block's rows of a counts matrix (30 % nonzero, values below 2^40) and 2,000 (row, column)
    pairs, same-node pairs among them."""
    if name in EXTRA:
        return _make(name, **EXTRA[name]())
    if not (name[0] == "k" and name[1:].isdigit()):  # a seam case outside EXTRA
        return _make(name, **_seam_args(name))
    k = int(name[1:])
    return _make(name, *axes(k), SEED0 + k)


def dense(g):
    """The library's own rule: more than 64 arcs per node, self-loops aside."""
    loops = int((g["src"] == g["dst"]).sum())
    return (len(g["src"]) - loops) * (1 if g["directed"] else 2) > 64 * g["n"]


def oracle_rows(O, g, used, rows=None):
    """(rc, latency, loss, first failing pair) from the oracle."""
    return O.shortest_paths(g["n"], g["src"], g["dst"], g["lat"], g["loss"], g["directed"], np.asarray(used, np.uint32),
                            rows=rows, threads=4)


_REFS = {}


def refs(O, name):
    """The references of every stage of case `name`, computed once and shared: per view the
    oracle's rows, tree_ref's (pred, first_hop, first untight cell, tight in-arcs per cell),
    link_ref's loads and paths_ref's records of the pairs."""
    if name in _REFS:
        return _REFS[name]
    c = case(name)
    g, nodes = c["g"], c["nodes"]
    out = []
    for v in c["views"]:
        rows = v["rows"]
        rc, lat, loss, first = oracle_rows(O, g, nodes, rows)
        r = dict(rc=rc, first=first, lat=lat, loss=loss)
        if rc == 0:
            r["pred"], r["hop"], r["bad"], r["tight"] = TR.tree_ref(g, nodes, rows, lat, loss, counts=True)
            if r["bad"] is None:
                r["link"], r["node"] = LR.link_load(g, nodes, rows, r["pred"], v["counts"])
                r["records"] = PR.records(g, nodes, rows, r["pred"], lat, loss, v["pairs"][0].astype(np.int64),
                                          v["pairs"][1])
        out.append(r)
    _REFS[name] = out
    return out


def round_refs(c, v, r, status, weight):
    """(link, node, hops) of link_round_ref for one view of a case."""
    return RR.link_load_round(c["g"], c["nodes"], v["rows"], r["pred"], c["hosts"], v["pk"], status, weight)


# ---- graphs that are not one strongly connected piece -------------------------------------------
def join(a, b):
    """a and b side by side, b's nodes renumbered after a's."""
    return dict(n=a["n"] + b["n"], src=np.concatenate([a["src"], b["src"] + a["n"]]).astype(np.uint32),
                dst=np.concatenate([a["dst"], b["dst"] + a["n"]]).astype(np.uint32),
                lat=np.concatenate([a["lat"], b["lat"]]), loss=np.concatenate([a["loss"], b["loss"]]),
                directed=a["directed"])


def _one_way(g, n_a, n_arcs, seed):
    """n_arcs arcs of 5 ms from the first n_a nodes to the nodes after them."""
    rng = np.random.default_rng(seed)
    cs, cd = rng.integers(0, n_a, n_arcs), rng.integers(n_a, g["n"], n_arcs)
    return dict(g, src=np.concatenate([g["src"], cs]).astype(np.uint32), dst=np.concatenate([g["dst"], cd]).astype(np.uint32),
                lat=np.concatenate([g["lat"], np.full(n_arcs, 5_000_000, np.uint64)]),
                loss=np.concatenate([g["loss"], np.zeros(n_arcs, np.float32)]))


NA, NB, N_ISLANDS = 600, 100, 703


@functools.lru_cache(maxsize=None)
def islands(directed):
    """A = ring_chords_graph(600, 6) and B = ring_chords_graph(100, 4) side by side (nodes 0 ..
    599 and 600 .. 699) and three isolated nodes without a self-loop (700 .. 702).  Directed: A
    and B both ways each, and 40 one-way arcs A -> B."""
    g = join(synth.ring_chords_graph(NA, 6.0, seed=3, directed=directed),
             synth.ring_chords_graph(NB, 4.0, seed=4, directed=directed))
    if directed:
        g = _one_way(g, NA, 40, 2)
    return dict(g, n=N_ISLANDS)


HALF = 66


@functools.lru_cache(maxsize=None)
def dense_blocks():
    """D: two complete directed blocks of 66 nodes (65 out-arcs per node: dense by the library's
    rule), a self-loop per node, 40 one-way arcs from the first block to the second."""
    rng = np.random.default_rng(17)
    i, j = np.nonzero(~np.eye(HALF, dtype=bool))
    v = np.arange(2 * HALF)
    src, dst = np.concatenate([v, i, i + HALF]), np.concatenate([v, j, j + HALF])
    m = len(src)
    g = dict(n=2 * HALF, src=src.astype(np.uint32), dst=dst.astype(np.uint32),
             lat=rng.integers(1, 301, m).astype(np.uint64) * 1_000_000, loss=synth._loss(rng, m), directed=True)
    g = _one_way(g, HALF, 40, 18)
    assert dense(g)
    return g


def _perm(seed, n, k=None):
    return np.random.default_rng(seed).permutation(n)[:k].astype(np.uint32)


def _ident(a, b):
    return np.arange(a, b, dtype=np.uint32)


def split_cases():
    """The builds that succeed, every used pair being connected whatever else the graph holds:
    name -> (graph, used list, row block or None for the whole table)."""
    und, di, d = islands(False), islands(True), dense_blocks()
    return {
        "S1_identity": (und, _ident(0, NA), None),
        "S1_identity_rows": (und, _ident(0, NA), (200, 450)),
        "S1_shuffled": (und, _perm(6, NA, 401), None),
        "S1_shuffled_rows": (und, _perm(6, NA, 401), (130, 300)),
        "S2_used_A": (di, _ident(0, NA), None),  # B is a reachable dead end
        "S2_used_A_rows": (di, _ident(0, NA), (200, 450)),
        "S2_used_B": (di, _ident(NA, NA + NB), None),  # A is unreachable and unused
        "S2_used_B_shuffled_rows": (di, (NA + _perm(7, NB)).astype(np.uint32), (30, 81)),
        "D_used_first": (d, _ident(0, HALF), None),
        "D_used_second": (d, _ident(HALF, 2 * HALF), None),
        "D_used_second_shuffled_rows": (d, (HALF + _perm(8, HALF)).astype(np.uint32), (11, 50)),
    }


def error_cases():
    """The builds that fail with SG_ERR_UNREACHABLE: name -> (graph, used, row block or None)."""
    und, di, d = islands(False), islands(True), dense_blocks()
    return {
        "E1": (und, _perm(1, NA + NB, 500), None),
        "E1_rows": (und, _perm(1, NA + NB, 500), (100, 200)),
        "E2_identity": (di, _ident(0, NA + NB), None),
        "E2_shuffled": (di, _perm(5, NA + NB), None),
        "D_identity": (d, _ident(0, 2 * HALF), None),
        "D_shuffled": (d, _perm(9, 2 * HALF), None),
    }


@functools.lru_cache(maxsize=None)
def second_graph():
    """The second net of the builds that follow a failing one."""
    return synth.ring_chords_graph(300, 6.0, seed=21)


def follow_up(name):
    """(graph or None for the failing build's own, used list) of the valid build after the
    failing build `name`: a used list of the other kind (an identity list after a shuffled one
    and the reverse), the same net and the second net in turn."""
    return {
        "E1": (None, _ident(0, NA)),
        "E1_rows": (second_graph(), _ident(0, 300)),
        "E2_identity": (None, _perm(6, NA, 401)),
        "E2_shuffled": (second_graph(), _ident(0, 300)),
        "D_identity": (second_graph(), _perm(11, 300, 211)),
        "D_shuffled": (None, _ident(0, HALF)),
    }[name]


# ---- the hop-record scan's second trip ----------------------------------------------------------
SCAN_TILE, SCAN_TRIP = 2048, 1024
SCAN_PAIRS = SCAN_TRIP * SCAN_TILE + 1


def scan_pairs(n, n_pairs=SCAN_PAIRS, seed=81):
    """Uniform pairs on n nodes; the last one a same-node pair (one record)."""
    rng = np.random.default_rng(seed)
    ri, cj = rng.integers(0, n, n_pairs).astype(np.uint32), rng.integers(0, n, n_pairs).astype(np.uint32)
    cj[-1] = ri[-1]
    return ri, cj


def walk_records(g, nodes, rows, pred, ri, cj):
    """(off u64, node u32, link u32) of the pairs, all pairs advancing one hop per step (as
    link_ref.link_load advances cells): first the hop counts, then every path written backwards
    from its last record."""
    n = g["n"]
    nodes = np.asarray(nodes, np.int64)
    r0, r1 = rows
    pred = np.asarray(pred, np.int64).reshape(r1 - r0, n)
    pred_by = np.empty_like(pred)
    pred_by[:, nodes] = pred
    _, _, keys = LR.links(g)
    row = np.asarray(ri, np.int64) - r0
    src, dst = nodes[np.asarray(ri, np.int64)], nodes[np.asarray(cj, np.int64)]
    same = src == dst
    cnt = same.astype(np.int64)
    cur, live = dst.copy(), np.flatnonzero(~same)
    for _ in range(n):
        if not len(live):
            break
        cnt[live] += 1
        cur[live] = pred_by[row[live], cur[live]]
        live = live[cur[live] != src[live]]
    assert not len(live), "a pred row that does not reach its source"
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    total = int(off[-1])
    node, link = np.zeros(total, np.uint32), np.zeros(total, np.uint32)
    at = off[1:].astype(np.int64) - 1  # the last record of every pair
    cur, live = dst.copy(), np.arange(len(src))
    while len(live):
        head = cur[live]
        tail = np.where(same[live], head, pred_by[row[live], head])
        k = LR.link_index(keys, tail, head)
        assert (k >= 0).all(), "a path step that is not a link"
        node[at[live]], link[at[live]] = head, k
        at[live] -= 1
        cur[live] = tail
        live = live[tail != src[live]]
    return off, node, link
