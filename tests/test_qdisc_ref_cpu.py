"""The reference model of the interface's qdiscs (tests/qdisc_ref.py) against the oracle where
the two must agree -- fifo, and round-robin with one socket per host or a socket per packet,
which is the fifo order -- and against orders worked by hand from the reference's rules
(interface.rs:168-181, :227-259; relay/mod.rs:111-273)."""
import numpy as np
import pytest

import qdisc_cases as qc
from qdisc_ref import FIFO, ROUND_ROBIN, Interfaces, QdiscError
from shadow_amd import synth

T0, MS = qc.T0, qc.MS
RELAY = ("rflags", "task_time", "task_id", "task_born", "tb_cap", "tb_bal", "tb_inc", "tb_last")


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("bw_mbit", [1000, 10, 2])
@pytest.mark.parametrize("mode", ["fifo", "one_socket", "socket_per_packet"])
def test_model_matches_oracle(oracle, mode, bw_mbit, keyed):
    """Random windows, unthrottled to heavily throttled, a bootstrap end inside the second one:
    statuses, forward times, counters, the sent batch and the relay state, window by window."""
    H, W, per, S = 150, 2 * MS, 3000, 256
    hosts = synth.make_hosts(H, 64, exact_seeds=False)
    rng = np.random.default_rng(bw_mbit)
    bw = rng.integers(bw_mbit * 10**6 // 2, bw_mbit * 10**6 + 1, H).astype(np.uint64)
    ost = oracle.outbound_state(hosts["ip"], bw, 512)
    m = Interfaces(hosts["ip"], bw, 512, FIFO if mode == "fifo" else ROUND_ROBIN,
                   S if mode == "socket_per_packet" else 1)
    n_pk = 3 * per
    fwd = [np.full(n_pk, np.uint64(2**64 - 1)) for _ in range(2)]
    st = [np.zeros(n_pk, np.uint8) for _ in range(2)]
    ctr = [np.full(H, 7, np.uint64) for _ in range(2)]
    seq = np.zeros(H, np.int64)  # socket_per_packet: the host's next slot
    boot, sim_end = T0 + 3 * MS, T0 + 10**12
    for w in range(3):
        t0, t1 = T0 + w * W, T0 + (w + 1) * W
        if keyed:
            host, t, ln, pay, dst, sock, eid, born = qc.keyed_sends(hosts, per, t0, t1, 50 * bw_mbit + w, 1)
        else:
            host, t, ln, pay, dst, sock = qc.sends(hosts, per, t0, t1, 100 * bw_mbit + w, 1)
            eid = born = None
        if mode == "socket_per_packet":
            rank = np.arange(per) - np.searchsorted(host, host)
            sock = ((seq[host] + rank) % S).astype(np.uint32)
            seq += np.bincount(host, minlength=H)
        pkt = np.arange(w * per, (w + 1) * per, dtype=np.uint32)
        want = oracle.outbound_run(ost, host, t, pkt, ln, pay, dst, t1, boot, sim_end, ctr[0], fwd[0], st[0],
                                   event_id=eid, event_created=born)
        got = m.run(host, t, pkt, ln, pay, dst, sock, t1, boot, sim_end, ctr[1], fwd[1], st[1],
                    event_id=eid, event_created=born)
        assert np.array_equal(st[0], st[1])
        assert np.array_equal(fwd[0], fwd[1])
        assert np.array_equal(ctr[0], ctr[1])
        for k in ("src_host", "dst_ipv4", "payload_len", "send_time", "packet"):
            assert np.array_equal(got[k], want[k]), k
        rs = m.relay_state()
        for k in RELAY:
            assert np.array_equal(rs[k], ost[k]), k
        if mode == "socket_per_packet":
            q = m.qdisc_state()
            assert q["active_count"].max(initial=0) <= 1
            assert np.array_equal(q["n_queued"], ost["tail"] - ost["head"])
    if bw_mbit == 2:
        assert (st[0] == 0).any() and (ost["rflags"] & oracle.RL_CACHED).any()
    assert (st[0] == 2).any()


@pytest.mark.parametrize("name", sorted(qc.HAND_CASES))
def test_hand_worked_orders(oracle, name):
    case = qc.HAND_CASES[name]
    host, t, pkt, ln, pay, dst, sock, eid, born = qc.hand_arrays(case)
    for qdisc, order in ((ROUND_ROBIN, case["order"]), (FIFO, case["fifo"])):
        m = Interfaces([10], [8 * 10**6], 16, qdisc, 4)
        ctr = np.full(1, case.get("ctr0", 0), np.uint64)
        fwd, st = np.zeros(len(pkt), np.uint64), np.zeros(len(pkt), np.uint8)
        out = m.run(host, t, pkt, ln, pay, dst, sock, case["end"], 0, T0 + 10**12, ctr, fwd, st, eid, born)
        assert list(out["packet"]) == order, qdisc
        assert list(out["packet"][np.argsort(out["send_time"], kind="stable")]) == order
        assert (st == 1).all() and m.hosts[0].n == 0
    # the fifo order is the oracle's
    ost = oracle.outbound_state([10], [8 * 10**6], 16)
    ctr = np.full(1, case.get("ctr0", 0), np.uint64)
    want = oracle.outbound_run(ost, host, t, pkt, ln, pay, dst, case["end"], 0, T0 + 10**12, ctr,
                               np.zeros(len(pkt), np.uint64), np.zeros(len(pkt), np.uint8), event_id=eid,
                               event_created=born)
    assert list(want["packet"]) == case["fifo"]


def test_canonical_state_lists_the_deque_and_the_cached_packet():
    """After A1 A2 B1 meet a blocked relay at one time: A1 is cached, the deque is [B, A]."""
    case = qc.HAND_CASES["cached_packets_socket_has_rotated"]
    host, t, pkt, ln, pay, dst, sock, _, _ = qc.hand_arrays(case)
    m = Interfaces([10], [8 * 10**6], 16, ROUND_ROBIN, 4)
    m.run(host, t, pkt, ln, pay, dst, sock, T0 + MS, 0, T0 + 10**12, np.zeros(1, np.uint64),
          np.zeros(4, np.uint64), np.zeros(4, np.uint8))
    q = m.qdisc_state()
    assert q["n_active"][0] == 2 and list(q["active"][:2]) == [qc.B, qc.A] and list(q["active_count"][:2]) == [1, 1]
    assert q["n_queued"][0] == 2 and list(q["q_packet"][:2]) == [3, 2]
    assert (q["cached_packet"][0], q["cached_len"][0], q["cached_dst"][0]) == (1, 1500, 11)
    assert m.relay_state()["rflags"][0] == 1 | 4


def test_model_errors():
    m = Interfaces([10], [8000], 2, ROUND_ROBIN, 2)
    z = lambda n: (np.zeros(1, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint8))
    one = lambda v, dt=np.uint32: np.array(v, dt)
    with pytest.raises(QdiscError) as e:  # a socket past max_sockets
        m.run(one([0]), one([T0], np.uint64), one([0]), one([100]), one([60]), one([11]), one([2]), T0 + MS, 0,
              T0 + 10**12, *z(1))
    assert e.value.code == -8
    with pytest.raises(QdiscError) as e:  # three sends into a pool of two
        m.run(one([0] * 3), one([T0] * 3, np.uint64), one([0, 1, 2]), one([1500] * 3), one([60] * 3), one([11] * 3),
              one([0, 1, 0]), T0 + MS, 0, T0 + 10**12, *z(3))
    assert e.value.code == -2
