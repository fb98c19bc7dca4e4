"""Rounds of the link-trace tests (test_trace_ref_cpu.py qualifies them on the CPU,
test_trace_gpu.py runs them).  Graphs, hosts and the other batches are those of
tests/tree_cases.py, tests/link_cases.py and tests/link_round_cases.py."""
import numpy as np

from shadow_amd import synth

import link_cases as LC
import link_round_cases as RC
import tree_cases as TC

T0 = RC.T0
SENT_OFF = np.uint64(0xA5A5A5A5A5A5A5A5)
SENT32 = np.uint32(0x5A5A5A5A)
SENT64 = np.uint64(0x5A5A5A5A00000000)

# (b): SG_LINK_TRACE_PIECE for the tier cases, and the library's default
PIECE, PIECE_DEFAULT = 128, 2048


def tier_lengths(piece):
    """(b): under, at and over one wave; around one piece; two pieces and a record, three pieces
    less one."""
    return [1, 63, 64, 65, piece - 1, piece, piece + 1, 2 * piece + 1, 3 * piece - 1]


def tie_round():
    """(a): 10,000 packets on the tie graph: 5,000 drawn as link_round_cases draws them, each sent
    twice, at one of four send times 250 us apart (all inside link_round_cases' round).  The
    twins share their path and their times, so every record's key differs from its twin's in
    the packet alone; the graph's latencies are whole milliseconds, so packets of other pairs
    sent at the same time tie with them as well.
    Returns (hosts, packets, mixed statuses): the statuses are drawn per pair of twins."""
    hosts = synth.make_hosts(1000, 300)
    pk = RC.batch(5000, hosts, 31)
    pk = {k: np.repeat(v, 2) for k, v in pk.items()}
    rng = np.random.default_rng(32)
    pk["send_time"] = np.repeat(np.uint64(T0) + rng.integers(0, 4, 5000).astype(np.uint64) * np.uint64(250_000), 2)
    return hosts, pk, np.repeat(RC.mixed_status(5000), 2)


def tier_graph():
    """(b): the path 0 - 1 - 2 (a self-loop per node, 1 ms arcs)."""
    return LC.path_graph(3)


def tier_round(n, shuffled):
    """(b): a host per node; n packets from the host at node 0 to the host at node 2, so links
    (0, 1) and (1, 2) hold n records each.  All send times equal (the order is by packet alone),
    or distinct and shuffled."""
    hosts = synth.make_hosts(3, 3)
    t = np.full(n, T0, np.uint64)
    if shuffled:
        t += np.random.default_rng(n).permutation(n).astype(np.uint64)
    return hosts, dict(src=np.zeros(n, np.uint32), dst_ip=np.full(n, hosts["ip"][2], np.uint32),
                       payload=np.zeros(n, np.uint32), send_time=t)


def wide_round(n_packets=3000, seed=51):
    """(f): four hosts per node of the 48-node ring with 1-3 s arcs; send times uniform below
    2^33 ns, so a link's enter times lie on both sides of 2^32."""
    hosts = synth.make_hosts(192, 48)
    pk = RC.batch(n_packets, hosts, seed)
    pk["send_time"] = np.random.default_rng(seed + 1).integers(0, 1 << 33, n_packets).astype(np.uint64)
    return hosts, pk


def wide_graph():
    return TC.wide_graph()


# (m): link counts one below, at and one past one tile of the link counters' scan (sweep_cases
# SCAN_TILE = 2048) -> (nodes, self-loops) of scan_edge_graph: 2 (n - 1) + k links
SCAN_EDGE = {2047: (1024, 1), 2048: (1025, 0), 2049: (1025, 1)}
SCAN_EDGE_ROWS = 32


def scan_edge_graph(n, k):
    """(m): the undirected path 0 - 1 - ... - n-1 with 1 ms arcs, self-loops on the first k nodes only."""
    v = np.arange(n)
    src = np.concatenate([v[:k], v[:-1]])
    dst = np.concatenate([v[:k], v[1:]])
    return LC._graph(n, src, dst, np.full(len(src), 1_000_000))


def scan_edge_round(n, n_packets=500, seed=61):
    """(m): the node order j -> 37 j mod n (a permutation: 37 divides neither 1024 nor 1025), so
    rows [0, SCAN_EDGE_ROWS) are sources spread along the path; a host per route index; packets
    from the hosts of those rows to hosts anywhere but the sender's own (no self-loop is crossed:
    most nodes have none).  Returns (nodes, hosts, packets)."""
    nodes = ((np.arange(n, dtype=np.int64) * 37) % n).astype(np.uint32)
    hosts = synth.make_hosts(n, n)
    rng = np.random.default_rng(seed)
    src = np.sort(rng.integers(0, SCAN_EDGE_ROWS, n_packets))
    dst = rng.integers(0, n - 1, n_packets)
    dst += dst >= src
    pk = dict(src=src.astype(np.uint32), dst_ip=hosts["ip"][dst].astype(np.uint32), payload=np.zeros(n_packets, np.uint32),
              send_time=np.uint64(T0) + rng.integers(0, 1_000_000, n_packets).astype(np.uint64))
    return nodes, hosts, pk


def scan_edge_tables(nodes):
    """(m): (pred, latency_ns) rows [0, SCAN_EDGE_ROWS) of the path, written out: the routing build
    refuses a used node without a self-loop, and a path has one tree per source anyway -- a node's
    predecessor is its neighbour towards the source, 1 ms a hop.  (The diagonal cell, a self-loop's
    latency, is left 0: no packet of the round reads it.)"""
    v = np.asarray(nodes, np.int64)[None, :]
    s = np.asarray(nodes, np.int64)[:SCAN_EDGE_ROWS, None]
    return (v + np.sign(s - v)).astype(np.uint32), (np.abs(s - v) * 1_000_000).astype(np.uint64)
