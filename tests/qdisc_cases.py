"""Send generators shared by test_qdisc_ref_cpu.py and test_qdisc_gpu.py: test_outbound_gpu.py's
window and keyed-tie patterns with a socket per send."""
import numpy as np

from shadow_amd import synth

T0 = 946684800 * 10**9
MS = 10**6


def sends(hosts, n, t0, t1, seed, n_sock, p_local=0.05):
    """n sends in [t0, t1) grouped by host in time order, 5 % to the host's own address, each on
    one of n_sock socket slots: (host, time, len, payload, dst, socket)."""
    pk = synth.make_packets(n, hosts, t0, t1, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    loc = rng.random(n) < p_local
    dst = np.where(loc, hosts["ip"][pk["src"]], pk["dst_ip"]).astype(np.uint32)
    ln = (pk["payload"] + 40).astype(np.uint32)  # IPv4 + TCP headers
    # every slot is drawn, the low ones far more often (a host's few busy sockets beside many
    # quiet ones): with 64 slots drawn evenly nearly every queued packet has a socket to itself,
    # which is the fifo order
    sock = np.minimum(n_sock * rng.random(n) ** 3, n_sock - 1).astype(np.uint32)
    return pk["src"], pk["send_time"], ln, pk["payload"], dst, sock


def keyed_sends(hosts, n, t0, t1, seed, n_sock):
    """Half of the sends exactly on a refill boundary (T0 + k ms, where a blocked relay's wake-up
    falls), each made by a random event: a Packet event (id UINT64_MAX) or a Local one created up
    to 3 ms earlier with a random id; per (host, time) in execution order: Packet events first,
    then Local ones by (created, id)."""
    host, t, ln, pay, dst, sock = sends(hosts, n, t0, t1, seed, n_sock)
    rng = np.random.default_rng(seed + 7)
    snap = rng.random(n) < 0.5
    t = np.where(snap, (t - T0) // MS * MS + T0, t).astype(np.uint64)
    t = np.maximum(t, np.uint64(t0))
    pk = rng.random(n) < 0.2
    born = (t - rng.integers(0, 3 * MS, n).astype(np.uint64)).astype(np.uint64)
    born = np.where(rng.random(n) < 0.3, (born - T0) // MS * MS + T0, born).astype(np.uint64)  # wake births
    eid = rng.integers(0, 5000, n).astype(np.uint64)
    born = np.where(pk, np.uint64(0), born)
    eid = np.where(pk, np.uint64(2**64 - 1), eid)
    o = np.lexsort((eid, born, ~pk, t, host))  # host, time, Packet first, created, id
    return host[o], t[o], ln[o], pay[o], dst[o], sock[o], eid[o], born[o]


def hosts_reordered(n_hosts, a, b):
    """How many hosts' packets two sent batches list in different orders (over as many packets
    as both list: one discipline may have forwarded more than the other)."""
    d = 0
    for h in range(n_hosts):
        pa, pb = a["packet"][a["src_host"] == h], b["packet"][b["src_host"] == h]
        n = min(len(pa), len(pb))
        d += not np.array_equal(pa[:n], pb[:n])
    return d


# Hand-worked orders, one host (address 10) at 8 Mbit/s: the bucket refills 1000 B every ms and
# holds 2500 B, so a 1500-B packet at T0 + 1 leaves 1000 B and the next 1500-B one blocks until
# the refill at T0 + 1 ms.  A send is (time, packet, len, socket[, (event created, event id)]);
# `order` is the forward order the reference's rules give, `fifo` the fifo qdisc's.
P, A, B = 2, 0, 1  # sockets
U64 = 2**64 - 1
_PKT = (0, U64)    # sent by a Packet event


def _tie_case(key):
    return [(T0 + 1, 0, 1500, P, _PKT), (T0 + 2, 1, 1500, P, _PKT), (T0 + 3, 2, 100, A, _PKT),
            (T0 + 4, 3, 100, A, _PKT), (T0 + MS, 4, 100, B, key)]


HAND_CASES = {
    # A1 A2 B1 queue behind the blocked relay: the deque is [A, B]; A1, then A goes to the back
    "one_from_each_socket": dict(
        sends=[(T0 + 1, 0, 1500, P), (T0 + 2, 1, 1500, P), (T0 + 3, 2, 100, A), (T0 + 4, 3, 100, A),
               (T0 + 5, 4, 100, B)],
        end=T0 + 2 * MS, order=[0, 1, 2, 4, 3], fifo=[0, 1, 2, 3, 4]),
    # A1 B1 B2 B3 queued; the wake-up at 1 ms forwards the cached packet and A1 (A drains) and
    # blocks on B1 (B rotates, the deque is [B]); A sends again and joins behind B: [B, A].  At 2 ms
    # B1, B2 (B rotates behind A), A2 blocks; at 3 ms A2, B3.
    "drained_socket_rejoins_at_the_back": dict(
        sends=[(T0 + 1, 0, 1500, P), (T0 + 2, 1, 1500, P), (T0 + 3, 2, 400, A), (T0 + 4, 3, 400, B),
               (T0 + 5, 4, 400, B), (T0 + 6, 5, 400, B), (T0 + MS + 10, 6, 400, A)],
        end=T0 + 4 * MS, order=[0, 1, 2, 3, 4, 6, 5], fifo=[0, 1, 2, 3, 4, 5, 6]),
    # A1 A2 B1 sent at one time, before the task they wake: it pops A1 (A goes behind B) and
    # blocks on it.  The cached A1 leaves first at 1 ms, then B1: A had already rotated.
    "cached_packets_socket_has_rotated": dict(
        sends=[(T0 + 1, 0, 1500, P), (T0 + 2, 1, 1500, A), (T0 + 2, 2, 100, A), (T0 + 2, 3, 100, B)],
        end=T0 + 2 * MS, order=[0, 1, 3, 2], fifo=[0, 1, 2, 3]),
    # B1 is sent at the wake-up's own nanosecond by a Local event.  Created before the task
    # (T0 + 2, id 102): the send runs first, the deque is [A, B] when the task pops: A1 B1 A2.
    "tie_send_first": dict(sends=_tie_case((T0 + 1, 50)), end=T0 + 2 * MS, ctr0=100, order=[0, 1, 2, 4, 3],
                           fifo=[0, 1, 2, 3, 4]),
    # Created after it: the task drains A first, then B1's own task forwards it.
    "tie_task_first": dict(sends=_tie_case((T0 + 5, 200)), end=T0 + 2 * MS, ctr0=100, order=[0, 1, 2, 3, 4],
                           fifo=[0, 1, 2, 3, 4]),
}


def hand_arrays(case):
    """A hand case's sends as the arrays of a run: (host, time, packet, len, payload, dst, socket,
    event_id or None, event_created or None)."""
    s = case["sends"]
    n = len(s)
    keyed = len(s[0]) > 4
    col = lambda j, dt: np.array([x[j] for x in s], dt)
    return (np.zeros(n, np.uint32), col(0, np.uint64), col(1, np.uint32), col(2, np.uint32),
            np.full(n, 60, np.uint32), np.full(n, 11, np.uint32), col(3, np.uint32),
            np.array([x[4][1] for x in s], np.uint64) if keyed else None,
            np.array([x[4][0] for x in s], np.uint64) if keyed else None)
