"""Hosts, batches, statuses and weights of the per-packet link-load tests
(test_link_round_ref_cpu.py qualifies them on the CPU, test_link_round_gpu.py runs them).  The
graphs are those of tests/link_cases.py."""
import numpy as np

from shadow_amd import synth

import link_cases as LC

T0 = 946684800 * 10**9
ROUND_END = T0 + 10**6
SENT64 = LC.SENT64
SENT32 = np.uint32(0x5A5A5A5A)  # out_hops starts from this: every entry is written
UMAX = np.uint32(0xFFFFFFFF)
DELIVERED, DROP_LOSS, DROP_NO_DST, SIM_END = 0, 1, 2, 3


def batch(n_packets, hosts, seed, **kw):
    return synth.make_packets(n_packets, hosts, T0, ROUND_END, seed=seed, **kw)


def tie_round():
    """(a), (b), (c): 1000 hosts on the tie graph's 300 nodes, 20,000 packets."""
    hosts = synth.make_hosts(1000, 300)
    return hosts, batch(20000, hosts, 31)


def big_weights(n_packets, seed=41):
    """(b): payloads up to 2^32 - 1, the first two the extremes."""
    w = np.random.default_rng(seed).integers(0, 1 << 32, n_packets, dtype=np.uint64).astype(np.uint32)
    w[:2] = 0xFFFFFFFF, 0
    return w


def mixed_status(n_packets, seed=42):
    """(c): the four SG_PKT_* values, uniform."""
    return np.random.default_rng(seed).integers(0, 4, n_packets).astype(np.uint8)


def shuffled_round():
    """(d): a shuffled node order, 400 hosts on its first 120 columns, the batch in the two halves
    its two row blocks [0, 60) and [60, 120) send."""
    nodes = np.random.default_rng(21).permutation(300).astype(np.uint32)
    hosts = synth.make_hosts(400, 120)
    lo = np.flatnonzero(hosts["route"] < 60)
    hi = np.flatnonzero(hosts["route"] >= 60)
    return nodes, hosts, batch(3000, hosts, 43, src_hosts=lo), batch(3000, hosts, 44, src_hosts=hi)


def same_node_round(n):
    """(e): two hosts per node, every packet to the other host of its sender's node."""
    hosts = synth.make_hosts(2 * n, n)
    src = np.arange(2 * n, dtype=np.uint32)
    pk = dict(src=src, dst_ip=hosts["ip"][(src + n) % (2 * n)].astype(np.uint32),
              payload=(src + 1).astype(np.uint32), send_time=np.full(2 * n, T0, np.uint64))
    return hosts, pk


def path_round():
    """(f): a host per node of the 4096-node path, 2,000 packets from the hosts of rows [0, 64),
    the first of them from node 0 to node 4095: 4,095 hops."""
    hosts = synth.make_hosts(4096, 4096)
    pk = batch(2000, hosts, 45, src_hosts=np.arange(64))
    first = int(np.flatnonzero(pk["src"] == 0)[0])
    pk["dst_ip"][first] = hosts["ip"][4095]
    return hosts, pk


def star_round():
    """(f): a host per node of the 512-spoke star, 3,000 packets from the host of spoke 1."""
    hosts = synth.make_hosts(513, 513)
    return hosts, batch(3000, hosts, 46, src_hosts=[1])


def block_round(rows, n_hosts, n_packets, seed):
    """(g): hosts on the first `rows` nodes only."""
    hosts = synth.make_hosts(n_hosts, rows)
    return hosts, batch(n_packets, hosts, seed)


def c3_round():
    """(h): a host per node at C3, 50,000 packets from the hosts of rows [0, 512) to hosts anywhere."""
    hosts = synth.make_hosts(10000, 10000, exact_seeds=False)
    return hosts, batch(50000, hosts, 48, src_hosts=np.arange(512))


def sparse_address_round():
    """(i): 300 hosts on addresses spread over 2^32 (no dense window: the sorted table resolves),
    5 % of the packets to an address no host holds, their status DROP_NO_DST."""
    hosts = synth.make_hosts(300, 300)
    hosts["ip"] = (np.random.default_rng(1).permutation(2**20)[:300].astype(np.uint32) * 4000 + 7).astype(np.uint32)
    pk = batch(8000, hosts, 9, p_unknown_dst=0.05)
    status = np.where(np.isin(pk["dst_ip"], hosts["ip"]), DELIVERED, DROP_NO_DST).astype(np.uint8)
    return hosts, pk, status
