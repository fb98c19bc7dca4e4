"""Rounds sharded over a device group, for the group's link loads and link trace
(test_group_trace_ref_cpu.py qualifies them on the CPU, test_group_trace_gpu.py runs them).

A group shards a round by source row block: member m holds rows row_range(n_rows, W, m) and the
packets whose sender's route row lies there.  `split` cuts a batch that way; the members' batches
concatenated in member order are the batch the single-context reference (tests/trace_ref.py,
tests/link_round_ref.py) takes, and a record's member is recovered from the packet bases."""
import numpy as np

from shadow_amd import synth
from shadow_amd.dist import row_range

import link_cases as LC
import link_round_cases as RC
import trace_ref as XR

T0 = RC.T0
WORLDS = (2, 3, 8)
SENT8 = np.uint8(0x5A)
FAN_W = 3
FAN_LENGTHS = (0, 1, 63, 64, 65, 2049)  # 2049: one past the default piece, a member's own sort merges
# per-member segment lengths on the shared link: every value of FAN_LENGTHS, 0 beside 2049
FAN_CASES = ((2049, 0, 65), (1, 63, 64), (65, 2049, 0), (63, 1, 2049))


def blocks(n_rows, world):
    """[(row_begin, row_end)] per member."""
    return [row_range(n_rows, world, m)[:2] for m in range(world)]


def split(hosts, pk, status, n_rows, world, ranges=None):
    """The batch by owner: per member (packets, statuses or None, indices into `pk`), each member's
    packets in the batch's own order."""
    ranges = blocks(n_rows, world) if ranges is None else ranges
    row = np.asarray(hosts["route"], np.int64)[np.asarray(pk["src"], np.int64)]
    out = []
    for r0, r1 in ranges:
        idx = np.flatnonzero((row >= r0) & (row < r1))
        out.append(({k: v[idx] for k, v in pk.items()}, None if status is None else np.asarray(status)[idx], idx))
    assert sum(len(x[2]) for x in out) == len(pk["src"]), "a sender outside every block"
    return out


def concat(parts):
    """(packets, statuses or None, bases) of the members' batches in member order."""
    pk = {k: np.concatenate([p[0][k] for p in parts]) for k in parts[0][0]}
    status = None if parts[0][1] is None else np.concatenate([p[1] for p in parts])
    sizes = [len(p[0]["src"]) for p in parts]
    return pk, status, np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint32)


def members_of(packet, bases):
    """The member of every record, from its packet index in the concatenated batch."""
    return (np.searchsorted(np.asarray(bases, np.int64), np.asarray(packet, np.int64), side="right") - 1).astype(np.uint8)


def trace(g, nodes, n_rows, pred, lat, hosts, parts, watch=None, bases=None):
    """(link_off, packet, member, hop, enter, exit) of the group's trace: trace_ref on the
    concatenated batch over all rows.  With explicit bases the packet numbers are rebased (the
    order is by (enter, member, local packet) whatever they are)."""
    pk, status, own = concat(parts)
    off, packet, hop, enter, leave = XR.trace(g, nodes, (0, n_rows), pred, lat, hosts, pk, status, watch)
    member = members_of(packet, own)
    if bases is not None:
        packet = (packet - own[member] + np.asarray(bases, np.uint32)[member]).astype(np.uint32)
    return off, packet, member, hop, enter, leave


def shared(g, nodes, n_rows, pred, lat, hosts, parts):
    """(links holding records of two or more members, (link, enter) groups holding records of two
    or more members) of the group's trace."""
    off, packet, member, _, enter, _ = trace(g, nodes, n_rows, pred, lat, hosts, parts)
    link = XR.segment_links(off)
    lm = np.unique(np.stack([link, member.astype(np.int64)]), axis=1)
    links = int((np.bincount(lm[0], minlength=len(off) - 1) >= 2).sum())
    _, inv = np.unique(np.stack([link, enter.astype(np.int64)]), axis=1, return_inverse=True)
    gm = np.unique(np.stack([inv.ravel(), member.astype(np.int64)]), axis=1)
    groups = int((np.bincount(gm[0]) >= 2).sum())
    return links, groups


# ---- fan-in: one source per member, one destination
FAN_N = 2 * FAN_W  # a path of 6 nodes: sources 0, 1, 2, the destination at node 5


def fan_graph():
    return LC.path_graph(FAN_N)


def fan_nodes():
    """Rows 0, 2, 4 (the first of each member's two rows) are the path's nodes 0, 1, 2."""
    return np.array([0, 3, 1, 4, 2, 5], np.uint32)


def fan_round(lengths, times):
    """A host per row (host h on route row h).  Member m's source (the host of row 2 m, at node m)
    sends lengths[m] packets to the host at node 5, so the last link (4, 5) holds a segment of
    lengths[m] records from member m.  times: "equal" (one send time), "tied" (send times that
    make every record enter the last link at one time: the order there is by member, then packet)
    or "shuffled" (distinct enter times in random order).  Returns (hosts, per-member parts)."""
    nodes = fan_nodes()
    hosts = synth.make_hosts(FAN_N, FAN_N)  # host h: route row h, so its node is nodes[h]
    dst = hosts["ip"][int(np.flatnonzero(nodes == FAN_N - 1)[0])]
    rng = np.random.default_rng(sum(lengths))
    total = sum(lengths)
    stamp = rng.permutation(total).astype(np.uint64) * np.uint64(7)
    parts, at = [], 0
    for m, k in enumerate(lengths):
        t = np.full(k, T0, np.uint64)
        if times == "tied":  # node m is 4 - m arcs of 1 ms before node 4
            t += np.uint64(m * 1_000_000)
        elif times == "shuffled":
            t += np.uint64(m * 1_000_000) + stamp[at:at + k]
        at += k
        pk = dict(src=np.full(k, 2 * m, np.uint32), dst_ip=np.full(k, dst, np.uint32), payload=np.zeros(k, np.uint32),
                  send_time=t)
        parts.append((pk, None, None))
    return hosts, parts


# ---- empty members: 3 nodes, 8 members
def tiny_graph():
    return LC.path_graph(3)


def tiny_round(n_packets=60, seed=5):
    """3 hosts on 3 rows; with 8 members rows 0, 1, 2 go to members 0, 1, 2 and five members have
    none."""
    hosts = synth.make_hosts(3, 3)
    return hosts, RC.batch(n_packets, hosts, seed)
