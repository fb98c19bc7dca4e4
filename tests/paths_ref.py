"""Batched tree paths, the definition restated in numpy (include/shadow_gpu.h, "batched tree
paths").  Deliberately not the library's algorithm: the library counts,
scans and fills backwards; here every pair's path is expanded on its own from its destination
and reversed on the host, its links are numbered through tests/link_ref.py link_index, and its
latencies and losses are gathered from the table the caller passes (the oracle's).  The expansion
is tests/tree_ref.py expand's walk with the column index built once per call instead of once per
pair (expand rebuilds it per call: 50,000 packets at 10,000 nodes would take minutes); every call
checks it against expand itself on its first EXPAND_CHECK distinct pairs.

A hop record is one link crossed: for row i (s = nodes[i]) and column j (d = nodes[j] != s) the
path s = v0 .. vh = d gives h records in source-to-destination order, record k = (vk, the link
(v(k-1), vk), lat[i][pos[vk]], loss[i][pos[vk]]); d == s gives one record (s, the link (s, s), the
diagonal cell); a packet that does not count gives none.
"""
import numpy as np

import link_ref as LR
import link_round_ref as RR
import tree_ref as TR

EXPAND_CHECK = 500


def records(g, nodes, rows, pred, tab_lat, tab_loss, ri, cj):
    """(off u64 [len + 1], node u32, link u32, latency_ns u64, packet_loss f32) of the pairs
    (ri[p], cj[p]) (rows absolute); a pair with ri[p] < 0 has no record."""
    n = g["n"]
    nodes = np.asarray(nodes, np.int64)
    pos = np.empty(n, np.int64)
    pos[nodes] = np.arange(n)
    r0, r1 = rows
    pred = np.asarray(pred, np.int64).reshape(r1 - r0, n)
    tab_lat = np.asarray(tab_lat, np.uint64).reshape(r1 - r0, n)
    tab_loss = np.asarray(tab_loss, np.float32).reshape(r1 - r0, n)
    _, _, keys = LR.links(g)
    pos_l, pred_l = pos.tolist(), {}
    off, heads, tails, rrow = [0], [], [], []
    seen = set()
    for i, j in zip(np.asarray(ri).tolist(), np.asarray(cj).tolist()):
        if i >= 0:
            assert r0 <= i < r1, "a pair outside the row block"
            s, d = int(nodes[i]), int(nodes[j])
            if d == s:
                path = [s, s]
            else:
                row = pred_l.get(i)
                if row is None:
                    row = pred_l[i] = pred[i - r0].tolist()
                path = [d]
                while path[-1] != s:
                    assert len(path) <= n, "the pred row does not reach the source"
                    path.append(row[pos_l[path[-1]]])
                path.reverse()
                if (i, j) not in seen and len(seen) < EXPAND_CHECK:
                    seen.add((i, j))
                    assert path == TR.expand(pred[i - r0], nodes, s, d), (i, j)
            heads.extend(path[1:])
            tails.extend(path[:-1])
            rrow.extend([i - r0] * (len(path) - 1))
        off.append(len(heads))
    heads, tails, rrow = np.asarray(heads, np.int64), np.asarray(tails, np.int64), np.asarray(rrow, np.int64)
    link = LR.link_index(keys, tails, heads) if len(heads) else np.zeros(0, np.int64)
    assert (link >= 0).all(), "a path step that is not a link"
    cols = pos[heads]
    return (np.asarray(off, np.uint64), heads.astype(np.uint32), link.astype(np.uint32), tab_lat[rrow, cols],
            tab_loss[rrow, cols])


def packet_pairs(hosts, pk, status):
    """(ri, cj) per packet, -1 where the packet does not count (link_round_ref.counted_pairs)."""
    n_packets = len(pk["src"])
    idx, r, c = RR.counted_pairs(hosts, pk, status)
    ri, cj = np.full(n_packets, -1, np.int64), np.full(n_packets, -1, np.int64)
    ri[idx], cj[idx] = r, c
    return ri, cj


def packet_records(g, nodes, rows, pred, tab_lat, tab_loss, hosts, pk, status=None):
    """records() of a round's batch: row = the sender's route index, column = the route index of
    the host the destination address resolves to; status None: every packet counts."""
    ri, cj = packet_pairs(hosts, pk, status)
    return records(g, nodes, rows, pred, tab_lat, tab_loss, ri, cj)


def first_bad_pair(rows, n, ri, cj):
    """The pair index sg_tree_paths reports, or None: the smallest p whose row lies outside the
    block or whose column is not below n."""
    r0, r1 = rows
    for p, (i, j) in enumerate(zip(np.asarray(ri).tolist(), np.asarray(cj).tolist())):
        if not r0 <= i < r1 or j >= n:
            return p
    return None


def first_bad_pred(g, nodes, rows, pred, ri, cj, links=True):
    """The (row, col) either entry point reports for corrupted pred rows, or None.  Every pair
    with ri >= 0 and another node for destination walks from its destination.  Counting comes
    first and looks at values only: the walk fails at the first node whose pred value is >= n
    (col = that node's column) or, when n steps have not reached the source, at its destination
    column; the smallest such (row, col) over all pairs is reported.  Only when counting found
    nothing, and only with links=True (out_link requested), filling reports the smallest
    (row, col) of a (pred, node) pair on a walked path that is not a link (a same-node pair: its
    self-loop, col = its column)."""
    n = g["n"]
    nodes = np.asarray(nodes, np.int64)
    pos = np.empty(n, np.int64)
    pos[nodes] = np.arange(n)
    r0, r1 = rows
    pred = np.asarray(pred, np.int64).reshape(r1 - r0, n)
    keys = set(LR.links(g)[2].tolist())
    bad_count = bad_link = None
    for i, j in sorted(set((i, j) for i, j in zip(np.asarray(ri).tolist(), np.asarray(cj).tolist()) if i >= 0)):
        s, v = int(nodes[i]), int(nodes[j])
        if v == s:
            if (s << 32 | s) not in keys and (bad_link is None or (i, j) < bad_link):
                bad_link = (i, j)
            continue
        fail = None
        not_link = []
        for _ in range(n):
            u = int(pred[i - r0, pos[v]])
            if u >= n:
                fail = (i, int(pos[v]))
                break
            if (v << 32 | u) not in keys:
                not_link.append((i, int(pos[v])))
            v = u
            if v == s:
                break
        else:
            fail = (i, j)
        if fail is not None:
            if bad_count is None or fail < bad_count:
                bad_count = fail
        elif not_link and (bad_link is None or min(not_link) < bad_link):
            bad_link = min(not_link)
    if bad_count is not None:
        return bad_count
    return bad_link if links else None
