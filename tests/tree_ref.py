"""Shortest-path trees, the definition restated in numpy (include/shadow_gpu.h, "shortest-path
trees").  Independent of the library: f32 operations one at a time, each
rounded (numpy float32 arithmetic), latency in u64.

For a source s, key[v] = the table's (latency, loss bits) of (s, v), key[s] = (0, +0.0f).  An
in-arc u -> v (u != v, v != s, parallel edges each) is tight when key[u].lat + w.lat == key[v].lat
and fold(key[u].loss, 1f32 - w.loss) has key[v]'s loss bits.  pred[s][v] = the smallest u among
v's tight in-arcs, pred[s][s] = s; first_hop[s][v] = the node after s on the pred path to v.
"""
import numpy as np

NONE = np.uint32(0xFFFFFFFF)
ONE = np.float32(1)


def fold(a, om):
    """PathProperties::add's loss (graph/mod.rs:328) with the edge's 1f32 - loss given:
    1f32 - (1f32 - a) * om, every operation rounded to f32."""
    a = np.asarray(a, np.float32)
    om = np.asarray(om, np.float32)
    return (ONE - ((ONE - a).astype(np.float32) * om).astype(np.float32)).astype(np.float32)


def arcs(g):
    """(tail, head, latency u64, 1f32 - loss) of every arc, self-loops left out; an undirected
    edge gives both directions."""
    src, dst = np.asarray(g["src"], np.int64), np.asarray(g["dst"], np.int64)
    lat, loss = np.asarray(g["lat"], np.uint64), np.asarray(g["loss"], np.float32)
    keep = src != dst
    a, b, w, f = src[keep], dst[keep], lat[keep], loss[keep]
    if not g["directed"]:
        a, b = np.concatenate([a, b]), np.concatenate([b, a])
        w, f = np.concatenate([w, w]), np.concatenate([f, f])
    return a, b, w, (ONE - f).astype(np.float32)


def tree_ref(g, nodes, rows, tab_lat, tab_loss, counts=False):
    """pred, first_hop (uint32 [r1 - r0, n], petgraph indices, columns in `nodes` order) and the
    first untight cell (row, col) in row-major order (rows absolute; None when every cell has a
    tight in-arc), from rows [r0, r1) of the full-width table over `nodes`, a permutation of every
    node.  Cells without a tight in-arc get pred = 0xFFFFFFFF.  counts=True also returns the
    number of tight in-arcs per cell."""
    n = g["n"]
    nodes = np.asarray(nodes, np.int64)
    assert sorted(nodes.tolist()) == list(range(n)), "nodes must be a permutation of every node"
    r0, r1 = rows
    tab_lat = np.asarray(tab_lat, np.uint64).reshape(r1 - r0, n)
    tab_loss = np.asarray(tab_loss, np.float32).reshape(r1 - r0, n)
    a, b, w, om = arcs(g)
    pred = np.full((r1 - r0, n), NONE, np.uint32)
    hop = np.zeros((r1 - r0, n), np.uint32)
    cnt = np.zeros((r1 - r0, n), np.uint32)
    first_bad = None
    ident = np.arange(n, dtype=np.int64)
    for i in range(r1 - r0):
        s = int(nodes[r0 + i])
        kl = np.zeros(n, np.uint64)
        kf = np.zeros(n, np.float32)
        kl[nodes] = tab_lat[i]
        kf[nodes] = tab_loss[i]
        kl[s] = 0
        kf[s] = np.float32(0.0)
        with np.errstate(over="ignore"):
            s_lat = kl[a] + w
        tight = (s_lat == kl[b]) & (s_lat >= kl[a]) & (fold(kf[a], om).view(np.uint32) == kf[b].view(np.uint32)) & (b != s)
        p = np.full(n, np.int64(NONE), np.int64)
        np.minimum.at(p, b[tight], a[tight])
        p[s] = s
        if counts:
            c = np.bincount(b[tight], minlength=n)
            cnt[i] = c[nodes]
        bad = p == np.int64(NONE)
        if bad.any() and first_bad is None:
            first_bad = (r0 + i, int(np.flatnonzero(bad[nodes])[0]))
        # pointer jumping: children of s (and cells without a tight arc) are fixed points
        h = np.where((p == s) | bad, ident, p)
        h[s] = s
        while True:
            h2 = h[h]
            if np.array_equal(h2, h):
                break
            h = h2
        pred[i] = p[nodes].astype(np.uint32)
        hop[i] = h[nodes].astype(np.uint32)
    if counts:
        return pred, hop, first_bad, cnt
    return pred, hop, first_bad


def expand(pred_row, nodes, src, dst):
    """The node sequence src ... dst from one pred row (columns in `nodes` order)."""
    pos = {int(v): j for j, v in enumerate(np.asarray(nodes).tolist())}
    out = [int(dst)]
    while out[-1] != src:
        assert len(out) <= len(pos), "the pred row does not reach the source"
        out.append(int(pred_row[pos[out[-1]]]))
    return out[::-1]


def refold(g, path, want_lat=None, want_loss=None, arc_index=None):
    """The left fold default() + e1 + ... + ek along `path`.  Where parallel arcs join two
    nodes, any arc that keeps the fold on the targets want_lat[v] / want_loss[v] (arrays by
    node, optional) is taken, else the first one.  Returns (latency int, loss f32)."""
    if arc_index is None:
        arc_index = build_arc_index(g)
    lat, loss = 0, np.float32(0.0)
    for u, v in zip(path[:-1], path[1:]):
        cands = arc_index[(u, v)]
        pick = None
        for w, om in cands:
            l2, f2 = lat + w, fold(loss, om)
            if want_lat is None or (l2 == int(want_lat[v]) and
                                    np.float32(f2).view(np.uint32) == np.float32(want_loss[v]).view(np.uint32)):
                pick = (l2, np.float32(f2))
                break
        assert pick is not None, f"no arc {u} -> {v} keeps the fold on the table"
        lat, loss = pick
    return lat, loss


def build_arc_index(g):
    a, b, w, om = arcs(g)
    idx = {}
    for x, y, l, f in zip(a.tolist(), b.tolist(), w.tolist(), om):
        idx.setdefault((x, y), []).append((l, f))
    return idx
