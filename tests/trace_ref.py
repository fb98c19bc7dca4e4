"""The link trace, the definition restated in numpy (include/shadow_gpu.h, "link trace";
DESIGN.md section 3.10).  Deliberately not the library's algorithm: the library counts per link,
scans, fills in whatever order its adds give and sorts every link's segment on its own; here the
per-packet hop records of tests/paths_ref.py (node, link and cumulative latency per hop, each
path expanded on the host) are turned into (packet, hop, enter, exit) rows and put in order by
one np.lexsort over (link, enter, packet).

A trace record is one (counted packet p, link crossed): hop k of p's path s = v0 .. vh = d lies on
link (v(k-1), vk) with enter = send_time[p] + cum(v(k-1)), exit = send_time[p] + cum(vk), cum(v)
the table's latency of v in the sender's row and cum(s) = 0; a packet to its sender's own node
has one record on the self-loop link, hop 1, enter = send_time[p], exit = send_time[p] + the
diagonal cell.  Link L owns records [link_off[L], link_off[L + 1]) in ascending (enter, packet)
order; a link with watch[L] == 0 owns none.
"""
import numpy as np

import link_ref as LR
import link_round_ref as RR
import paths_ref as PR


def n_links(g):
    return len(LR.links(g)[0])


def unsorted_records(g, nodes, rows, pred, tab_lat, hosts, pk, status=None):
    """(link, packet, hop, enter, exit) of every crossing, grouped by packet in path order: the
    transpose's input.  The sums wrap as u64 sums do; first_overflow tells whether one does."""
    tab_lat = np.asarray(tab_lat, np.uint64)
    off, _, link, lat, _ = PR.packet_records(g, nodes, rows, pred, tab_lat, np.zeros(tab_lat.shape, np.float32), hosts, pk,
                                             status)
    cnt = np.diff(off.astype(np.int64))
    total = int(off[-1])
    packet = np.repeat(np.arange(len(cnt), dtype=np.int64), cnt)
    hop = np.arange(total, dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), cnt) + 1
    send = np.asarray(pk["send_time"], np.uint64)[packet]
    before = np.zeros(total, np.uint64)  # cum of the hop's tail: the record before it, 0 at the source
    later = np.flatnonzero(hop > 1)
    before[later] = lat[later - 1]
    with np.errstate(over="ignore"):
        enter, leave = send + before, send + lat
    return link.astype(np.int64), packet.astype(np.uint32), hop.astype(np.uint32), enter, leave


def watch_mask(g, watch):
    """A u8 mask per link from None (every link), a mask, or a list of link numbers."""
    nl = n_links(g)
    if watch is None:
        return np.ones(nl, np.uint8)
    w = np.asarray(watch)
    if w.dtype == np.bool_ or (w.dtype == np.uint8 and w.shape == (nl,)):
        assert w.shape == (nl,)
        return w.astype(np.uint8)
    m = np.zeros(nl, np.uint8)
    m[w.astype(np.int64)] = 1
    return m


def trace(g, nodes, rows, pred, tab_lat, hosts, pk, status=None, watch=None):
    """(link_off u64 [n_links + 1], packet u32, hop u32, enter_ns u64, exit_ns u64)."""
    link, packet, hop, enter, leave = unsorted_records(g, nodes, rows, pred, tab_lat, hosts, pk, status)
    keep = watch_mask(g, watch)[link] != 0
    link, packet, hop, enter, leave = link[keep], packet[keep], hop[keep], enter[keep], leave[keep]
    order = np.lexsort((packet, enter, link))
    off = np.concatenate([[0], np.cumsum(np.bincount(link, minlength=n_links(g)))]).astype(np.uint64)
    return off, packet[order], hop[order], enter[order], leave[order]


def segment_links(link_off):
    """The link number of every record of a trace."""
    return np.repeat(np.arange(len(link_off) - 1, dtype=np.int64), np.diff(np.asarray(link_off).astype(np.int64)))


def first_overflow(nodes, rows, tab_lat, hosts, pk, status=None):
    """The packet SG_ERR_TIME_OVERFLOW names, or None: the smallest counted packet whose
    send_time + latency[row][column] is past 2^64 - 1."""
    r0, r1 = rows
    tab_lat = np.asarray(tab_lat, np.uint64).reshape(r1 - r0, len(nodes))
    idx, ri, cj = RR.counted_pairs(hosts, pk, status)
    send = np.asarray(pk["send_time"], np.uint64)
    for p, i, j in zip(idx.tolist(), ri.tolist(), cj.tolist()):
        if int(send[p]) + int(tab_lat[i - r0, j]) >= 1 << 64:
            return p
    return None
