"""Link loads, the definition restated in numpy (include/shadow_gpu.h, "link loads"; DESIGN.md
section 3.7).  Deliberately not the library's algorithm: the library sums subtrees from the
leaves up; here every nonzero cell walks dst -> ... -> src up its row's pred, all cells at once,
one np.add.at per hop level, and adds its count to each link it passes.

A link is a distinct ordered node pair joined by an edge (an undirected edge gives both
directions, parallel edges one link, a self-loop (a, a)), in ascending (head, tail) order.
"""
import numpy as np

NONE = np.uint32(0xFFFFFFFF)


def links(g):
    """(tail, head, key): the link list and its sorted keys (head << 32) | tail."""
    src, dst = np.asarray(g["src"], np.uint64), np.asarray(g["dst"], np.uint64)
    keys = (dst << np.uint64(32)) | src
    if not g["directed"]:
        keys = np.concatenate([keys, (src << np.uint64(32)) | dst])
    keys = np.unique(keys)
    return (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), (keys >> np.uint64(32)).astype(np.uint32), keys


def link_index(keys, tail, head):
    """Index of the links (tail[k] -> head[k]); -1 where the pair is not a link."""
    want = (np.asarray(head, np.uint64) << np.uint64(32)) | np.asarray(tail, np.uint64)
    at = np.searchsorted(keys, want)
    at = np.minimum(at, max(len(keys) - 1, 0))
    ok = keys[at] == want if len(keys) else np.zeros(len(want), bool)
    return np.where(ok, at.astype(np.int64), -1)


def edge_links(g):
    """(fwd, rev) per edge: the link (src -> dst); the link (dst -> src), 0xFFFFFFFF when directed."""
    _, _, keys = links(g)
    fwd = link_index(keys, g["src"], g["dst"]).astype(np.uint32)
    if g["directed"]:
        return fwd, np.full(len(fwd), NONE, np.uint32)
    return fwd, link_index(keys, g["dst"], g["src"]).astype(np.uint32)


def link_load(g, nodes, rows, pred, counts, link=None, node=None):
    """Adds rows [r0, r1) into (link, node) (u64; zeros when not given) and returns them.
    pred: [r1 - r0, n] petgraph indices, columns in `nodes` order; counts: [r1 - r0, count_cols]."""
    n = g["n"]
    nodes = np.asarray(nodes, np.int64)
    r0, r1 = rows
    pred = np.asarray(pred, np.int64).reshape(r1 - r0, n)
    counts = np.asarray(counts, np.uint64).reshape(r1 - r0, -1)
    tail, head, keys = links(g)
    link = np.zeros(len(keys), np.uint64) if link is None else link
    node = np.zeros(n, np.uint64) if node is None else node
    ri, cj = np.nonzero(counts)
    c = counts[ri, cj]
    # by node: pred_by[i, v] = the predecessor of node v in row i
    pred_by = np.empty_like(pred)
    pred_by[:, nodes] = pred
    src = nodes[r0 + ri]
    cur = nodes[cj]
    diag = cur == src
    k = link_index(keys, src[diag], src[diag])
    assert (k >= 0).all(), "a diagonal count on a node without a self-loop"
    with np.errstate(over="ignore"):
        np.add.at(link, k, c[diag])
        ri, c, src, cur = ri[~diag], c[~diag], src[~diag], cur[~diag]
        for _ in range(n):
            if not len(cur):
                break
            p = pred_by[ri, cur]
            k = link_index(keys, p, cur)
            assert (k >= 0).all(), "a pred step that is not a link"
            np.add.at(link, k, c)
            np.add.at(node, cur, c)
            go = p != src
            ri, c, src, cur = ri[go], c[go], src[go], p[go]
        assert not len(cur), "a pred row that does not reach its source"
    return link, node


def first_bad(g, nodes, rows, pred, counts):
    """The (row, col) sg_link_load reports for corrupted rows, or None: per nonzero row, a value
    >= n or pred[s] != s first (the smaller column); else, the smaller column of a node with
    traffic whose (pred, node) is not a link and of a node that is never released (on a cycle)."""
    n = g["n"]
    nodes = np.asarray(nodes, np.int64)
    pos = np.empty(n, np.int64)
    pos[nodes] = np.arange(n)
    r0, r1 = rows
    pred = np.asarray(pred, np.int64).reshape(r1 - r0, n)
    counts = np.asarray(counts, np.uint64).reshape(r1 - r0, -1)
    _, _, keys = links(g)
    for i in range(r1 - r0):
        if not counts[i].any():
            continue
        s = int(nodes[r0 + i])
        cand = np.flatnonzero(pred[i] >= n).tolist()
        if pred[i, r0 + i] != s:
            cand.append(r0 + i)
        if cand:
            return (r0 + i, min(cand))
        par = np.empty(n, np.int64)
        par[nodes] = pred[i]
        # the nodes of cycles: the image of par iterated past n steps, the root's fixed point aside
        f = par.copy()
        for _ in range(int(np.ceil(np.log2(max(n, 2)))) + 1):
            f = f[f]
        cyc = set(np.unique(f).tolist()) - {s}
        cand = [int(pos[v]) for v in cyc]
        # subtree sums by Kahn's peeling, for "traffic crosses the pair"
        c = np.zeros(n, np.uint64)
        c[nodes[:counts.shape[1]]] = counts[i]
        c[s] = 0
        sub = c.copy()
        deg = np.bincount(par[np.arange(n) != s], minlength=n)
        stack = [v for v in range(n) if deg[v] == 0 and v != s]
        while stack:
            v = stack.pop()
            p = int(par[v])
            if sub[v] and link_index(keys, [p], [v])[0] < 0:
                cand.append(int(pos[v]))
            if p != s:
                sub[p] += sub[v]
                deg[p] -= 1
                if deg[p] == 0:
                    stack.append(p)
        if counts[i, r0 + i] if r0 + i < counts.shape[1] else 0:
            if link_index(keys, [s], [s])[0] < 0:
                cand.append(r0 + i)
        if cand:
            return (r0 + i, min(cand))
    return None
