"""Link loads from a round's packets, the definition restated in numpy (include/shadow_gpu.h,
"link loads from a round's packets").  Deliberately not the library's
algorithm: the library walks every packet's tree path; here the counted packets' weights are
summed into a dense (rows x n) u64 matrix, one cell per (source row, destination column), and
that matrix goes to the dense reference tests/link_ref.py link_load.  Hosts resolve through a
dict.  Hops come from a level-by-level walk of all packets at once, checked against
tests/tree_ref.py expand (length - 1; 1 for a same-node pair) on the first EXPAND_CHECK distinct
pairs: expand rebuilds its column index per call, which is too slow for every packet of the
larger cases.
"""
import numpy as np

import link_ref as LR
import tree_ref as TR

UMAX = np.uint32(0xFFFFFFFF)
DELIVERED = 0
EXPAND_CHECK = 200


def resolve(hosts, dst_ip):
    """Destination host per packet through a dict; -1 where no host holds the address."""
    ip_to_host = {int(ip): h for h, ip in enumerate(np.asarray(hosts["ip"]).tolist())}
    return np.array([ip_to_host.get(int(x), -1) for x in np.asarray(dst_ip).tolist()], np.int64)


def counted_pairs(hosts, pk, status):
    """(index, row, column) of the counted packets: status DELIVERED, or every packet."""
    n_packets = len(pk["src"])
    counts = np.ones(n_packets, bool) if status is None else np.asarray(status)[:n_packets] == DELIVERED
    idx = np.flatnonzero(counts)
    dh = resolve(hosts, pk["dst_ip"][idx])
    assert (dh >= 0).all(), "a counted packet to an unknown address"
    route = np.asarray(hosts["route"], np.int64)
    return idx, route[pk["src"][idx].astype(np.int64)], route[dh]


def hops_of(nodes, rows, pred, ri, cj):
    """Links crossed per (row, column) pair: 1 for a same-node pair, else the steps from the
    column's node up to the row's source."""
    n = len(nodes)
    nodes = np.asarray(nodes, np.int64)
    r0, r1 = rows
    pred = np.asarray(pred, np.int64).reshape(r1 - r0, n)
    pred_by = np.empty_like(pred)
    pred_by[:, nodes] = pred
    src, cur = nodes[ri], nodes[cj]
    hops = np.where(cur == src, 1, 0).astype(np.uint32)
    live = np.flatnonzero(cur != src)
    for _ in range(n):
        if not len(live):
            break
        hops[live] += 1
        cur[live] = pred_by[ri[live] - r0, cur[live]]
        live = live[cur[live] != src[live]]
    assert not len(live), "a pred row that does not reach its source"
    # the same from tree_ref.expand, on a sample
    seen = set()
    for k in range(len(ri)):
        key = (int(ri[k]), int(cj[k]))
        if key in seen:
            continue
        seen.add(key)
        path = TR.expand(pred[key[0] - r0], nodes, int(nodes[key[0]]), int(nodes[key[1]]))
        assert hops[k] == (1 if len(path) == 1 else len(path) - 1), key
        if len(seen) >= EXPAND_CHECK:
            break
    return hops


def link_load_round(g, nodes, rows, pred, hosts, pk, status=None, weight=None, link=None, node=None):
    """(link, node, hops): the counted packets' weights (1 when weight is None) added into
    (link, node) (u64; zeros when not given); hops u32 per packet, 0xFFFFFFFF where not counted."""
    n = g["n"]
    r0, r1 = rows
    n_packets = len(pk["src"])
    idx, ri, cj = counted_pairs(hosts, pk, status)
    assert ((ri >= r0) & (ri < r1)).all(), "a sender outside the row block"
    w = np.ones(len(idx), np.uint64) if weight is None else np.asarray(weight)[idx].astype(np.uint64)
    m = np.zeros((r1 - r0, n), np.uint64)
    with np.errstate(over="ignore"):
        np.add.at(m, (ri - r0, cj), w)
    link, node = LR.link_load(g, nodes, rows, pred, m, link, node)
    hops = np.full(n_packets, UMAX, np.uint32)
    hops[idx] = hops_of(nodes, rows, pred, ri, cj)
    return link, node, hops


def first_bad_packet(hosts, pk, status, rows, n):
    """The packet index sg_link_load_packets reports, or None: the smallest p whose source host
    is past the host table or whose source's route row lies outside the block (counted or not),
    or that counts and goes to an address no host holds or to a route index >= n."""
    r0, r1 = rows
    route = np.asarray(hosts["route"], np.int64)
    ip_to_host = {int(ip): h for h, ip in enumerate(np.asarray(hosts["ip"]).tolist())}
    for p in range(len(pk["src"])):
        h = int(pk["src"][p])
        if h >= len(route) or not r0 <= route[h] < r1:
            return p
        if status is None or status[p] == DELIVERED:
            d = ip_to_host.get(int(pk["dst_ip"][p]))
            if d is None or route[d] >= n:
                return p
    return None


def first_bad_pred(g, nodes, rows, pred, hosts, pk, status=None):
    """The (row, col) sg_link_load_packets reports for corrupted pred rows, or None: every counted
    packet walks from its destination; it fails at the first node whose pred value is >= n or
    whose (pred, node) pair is not a link (col = that node's column), or, when n steps have not
    reached the source, at its destination column.  The smallest (row, col) over all packets."""
    n = g["n"]
    nodes = np.asarray(nodes, np.int64)
    pos = np.empty(n, np.int64)
    pos[nodes] = np.arange(n)
    r0, r1 = rows
    pred = np.asarray(pred, np.int64).reshape(r1 - r0, n)
    links = set(LR.links(g)[2].tolist())
    idx, ri, cj = counted_pairs(hosts, pk, status)
    bad = None
    for i, j in sorted(set(zip(ri.tolist(), cj.tolist()))):
        s, v = int(nodes[i]), int(nodes[j])
        fail = None
        if v == s:
            if (s << 32 | s) not in links:
                fail = (i, j)
        else:
            for _ in range(n):
                u = int(pred[i - r0, pos[v]])
                if u >= n or (v << 32 | u) not in links:
                    fail = (i, int(pos[v]))
                    break
                v = u
                if v == s:
                    break
            else:
                fail = (i, j)
        if fail is not None and (bad is None or fail < bad):
            bad = fail
    return bad
