"""Graphs whose shortest-path optima land on the 2^32 ns seam of the searches' 32-bit keys by
construction (test_seam_ref_cpu.py qualifies them on the CPU; test_sweep_gpu.py, test_seam_gpu.py
and test_sssp_chain_gpu.py run them).

S = 2^32 - 1 is what a saturated 32-bit latency reads as: S - 1 is the largest latency a 32-bit
key holds as a real value, a row with a cell >= S has to be redone in 64 bits.  Every case is a
graph of sweep_cases.graph() (regimes "unit", "us" and "ms": far below the seam; u is the
regime's unit, 1,000 ns or 10^6 ns) plus a few nodes hung on a hub h whose arcs are sized from
the latency-only distances d0[.] from h (integer Bellman-Ford here, undirected edges mirrored),
so that chosen cells are exactly S - 3 .. S + 2.  Every added node has one self-loop of latency
u, no added arc is shorter than u, and the edge order is shuffled at the end.

Directed ("spur").  f and g2 are the farthest and second-farthest nodes from h, x = d0[f] - d0[g2].
  dn:   f -> dn (u, loss 0.5) is the optimum; g2 -> dn (x + u + 6, loss 0) is a decoy 6 ns later
        and lossless: once both saturate they read the same 32-bit latency and the decoy's loss
        is the smaller; dn -> h (u, loss 0).  E = d0[f] + u = d0[dn].
  s_e:  e in -3 .. 2: s_e -> h (S + e - E, loss spur_loss) and h -> s_e (u).  D[s_e][dn] = S + e,
        the maximum of row s_e.
  t_e:  e in -1 .. 1: t_e -> h of latency exactly S + e (the arc clamp itself on the seam) and
        h -> t_e (u).

Undirected ("under", "across").  lv is sorted d0 at index int(0.75 (n - 1)); s_e - h has latency
S + e - lv, so D[v][s_e] = S + e + d0[v] - lv.  "under" (e in -3 .. -1): rows of nodes at level lv
have maximum exactly S - 1, nearer nodes stay below, farther nodes and the spurs hold wide cells,
and no cell is in [S, S + 2].  "across" (e in -3 .. 2): cells of exactly S, S + 1, S + 2 sit in
rows that also hold narrow cells.
"""
import functools

import numpy as np

import sweep_cases as SC

S = (1 << 32) - 1
UNIT = {"unit": 1000, "us": 1000, "ms": 1_000_000}
SPUR_OFFS = (-3, -2, -1, 0, 1, 2)
ARC_OFFS = (-1, 0, 1)
OFFS = {"spur": SPUR_OFFS, "under": (-3, -2, -1), "across": SPUR_OFFS}

# name -> (kind, graph()'s n, directed, degree, latency regime, loss regime, spur_loss)
CASES = {
    "spur_us63": ("spur", 63, True, 3.0, "us", "four", 0.0),
    "spur_us200_lossy": ("spur", 200, True, 6.0, "us", "uniform", 0.01),
    "spur_dense": ("spur", 130, True, 80.0, "us", "four", 0.0),
    "under_ms129": ("under", 129, False, 6.0, "ms", "tie", 0.0),
    "across_ms129": ("across", 129, False, 6.0, "ms", "tie", 0.0),
    "under_dense": ("under", 130, False, 150.0, "ms", "tie", 0.0),
    "under_ms600": ("under", 600, False, 6.0, "ms", "zero", 0.0),
    "under_unit600": ("under", 600, False, 4.0, "unit", "half", 0.0),
}
DENSE = ("spur_dense", "under_dense")
SMALL = SC.SEAM  # the six that run through the sweep
CHAIN_ONLY = tuple(k for k in CASES if k not in SMALL)  # 600 nodes: for chained rows, not for the sweep
assert set(SMALL) <= set(CASES)


def distances(g, h):
    """Latency-only distances from h: integer Bellman-Ford, undirected edges mirrored."""
    src, dst, lat = g["src"].astype(np.int64), g["dst"].astype(np.int64), g["lat"].astype(np.int64)
    if not g["directed"]:
        src, dst, lat = np.concatenate([src, dst]), np.concatenate([dst, src]), np.concatenate([lat, lat])
    d = np.full(g["n"], np.iinfo(np.int64).max // 2, np.int64)
    d[h] = 0
    for _ in range(g["n"]):
        nd = d.copy()
        np.minimum.at(nd, dst, d[src] + lat)
        if np.array_equal(nd, d):
            break
        d = nd
    return d


@functools.lru_cache(maxsize=None)
def build(name):
    """The graph of case `name` and what it was built from: kind, u, h, d0 (of the base's nodes),
    the added nodes (spurs: e -> s_e; arc_spurs: e -> t_e; dn, f, g2 when directed) and, when
    undirected, lv and the base's nodes at that level.  Seeds: 4242 + n for graph(), that + 555 for
    the hub and the final shuffle (the conditions test_seam_ref_cpu.py asserts are the contract,
    not the seeds)."""
    kind, n, directed, degree, lat_regime, loss_regime, spur_loss = CASES[name]
    seed = 4242 + n
    g = SC.graph(n, directed, degree, lat_regime, loss_regime, seed)
    rng = np.random.default_rng(seed + 555)
    u = UNIT[lat_regime]
    h = int(rng.integers(n))
    d0 = distances(g, h)
    arcs = []  # (tail, head, latency, loss)
    info = dict(kind=kind, u=u, h=h, d0=d0)
    at = n
    if kind == "spur":
        order = np.argsort(d0, kind="stable")
        f, g2 = int(order[-1]), int(order[-2])
        x = int(d0[f] - d0[g2])
        dn, at = at, at + 1
        arcs += [(f, dn, u, 0.5), (g2, dn, x + u + 6, 0.0), (dn, h, u, 0.0)]
        reach = int(d0[f]) + u
        spurs, arc_spurs = {}, {}
        for e in SPUR_OFFS:
            spurs[e], at = at, at + 1
            arcs += [(spurs[e], h, S + e - reach, spur_loss), (h, spurs[e], u, 0.0)]
        for e in ARC_OFFS:
            arc_spurs[e], at = at, at + 1
            arcs += [(arc_spurs[e], h, S + e, 0.0), (h, arc_spurs[e], u, 0.0)]
        info.update(dn=dn, f=f, g2=g2, spurs=spurs, arc_spurs=arc_spurs)
    else:
        lv = int(np.sort(d0)[int(0.75 * (n - 1))])
        spurs = {}
        for e in OFFS[kind]:
            spurs[e], at = at, at + 1
            arcs.append((spurs[e], h, S + e - lv, 0.0))
        info.update(lv=lv, level=np.flatnonzero(d0 == lv), spurs=spurs, arc_spurs={})
    arcs += [(v, v, u, 0.0) for v in range(n, at)]
    assert min(a[2] for a in arcs) >= u
    src = np.concatenate([g["src"], np.array([a[0] for a in arcs], np.uint32)])
    dst = np.concatenate([g["dst"], np.array([a[1] for a in arcs], np.uint32)])
    lat = np.concatenate([g["lat"], np.array([a[2] for a in arcs], np.uint64)])
    loss = np.concatenate([g["loss"], np.array([a[3] for a in arcs], np.float32)])
    p = rng.permutation(len(src))
    info["g"] = dict(n=at, src=src[p], dst=dst[p], lat=lat[p], loss=loss[p], directed=directed)
    return info


def seam_rows(name):
    """(nodes whose row's maximum is in [S - 3, S - 1], nodes whose row holds a cell >= S), as far
    as the construction alone tells: enough of each to place the row block.  "across" has no row
    of the first kind (its level rows run on to S + 2): there both lists are the level rows, which
    hold the cells S - 3 .. S - 1 beside the cells S .. S + 2."""
    b = build(name)
    if b["kind"] == "spur":
        return [b["spurs"][e] for e in (-3, -2, -1)], [b["spurs"][e] for e in (0, 1, 2)] + list(b["arc_spurs"].values())
    if b["kind"] == "under":
        return b["level"].tolist(), list(b["spurs"].values())
    return b["level"].tolist(), b["level"].tolist()


def _block(name, nodes):
    """The case's second view: sweep_cases' block [n // 3, n - n // 4) of `nodes`, widened to the
    nearest row of either kind of seam_rows() that it lacks."""
    n = len(nodes)
    pos = np.empty(n, np.int64)
    pos[nodes] = np.arange(n)
    r0, r1 = n // 3, n - n // 4
    for kind in seam_rows(name):
        at = pos[np.asarray(kind, np.int64)]
        if ((at >= r0) & (at < r1)).any():
            continue
        below, above = at[at < r0], at[at >= r1]
        if len(below) and (not len(above) or r0 - below.max() <= above.min() + 1 - r1):
            r0 = int(below.max())
        else:
            r1 = int(above.min()) + 1
    return r0, r1


def make_args(name):
    """sweep_cases._make's arguments for case `name`."""
    kind, n, directed, degree, lat_regime, loss_regime, _ = CASES[name]
    return dict(n=n, directed=directed, degree=degree, lat_regime=lat_regime, loss_regime=loss_regime, seed=4242 + n,
                g=build(name)["g"], block=functools.partial(_block, name))
