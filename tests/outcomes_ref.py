"""A link-queue result folded onto its packets (sg_link_queue with its packets flag), the definition
restated (include/shadow_gpu.h, "link queues") as loops over Python integers.

Input is a queue result as queue_ref, queue_carry_ref or queue_drop_ref give it: per record wait and
done at the input indices, whose sentinels tell a record's state (served; dropped: wait 2^64 - 1,
done not; absent: both).  All times are the input enter times, not the carried ones.

Per packet p, over R(p), its records:
    drop(p)   the dropped record with the smallest (enter, index); t_drop its enter, else +infinity
    S(p)      the served records with enter < t_drop
    where     drop(p); ARRIVED when R(p) is not empty and has no dropped record; NOTHING when empty
    delay     carried: done - enter of the record of S(p) with the largest enter; first order: the
              sum of done - enter over S(p), wrapping; 0 when S(p) is empty
    arrive    2^64 - 1 when dropped, base + delay when arrived, base when R(p) is empty
Deliberately not the library's algorithm (a chain walk carried, a minimum and a sum by atomics first
order): plain loops, one packet after the other.
"""
import numpy as np

from queue_ref import INVALID_ARG, MAX, OK, TIME_OVERFLOW, bad_link_off  # noqa: F401

CAPACITY = 10
ARRIVED = 0xFFFFFFFE
NOTHING = 0xFFFFFFFF
# The flag's name, in two parts (queue_carry_cases.CARRY_FLAG tells why), and its value.
PACKETS_FLAG = "SG_LINK_" + "QUEUE_PACKETS"
PACKETS = 0x10


def state(wait, done):
    if wait != MAX:
        return "served"
    return "absent" if done == MAX else "dropped"


def outcomes(link_off, enter, packet, wait, done, n_packets, carry, base):
    """(status, records, delay, arrive, where).  INVALID_ARG: records is the smallest i with
    packet[i] >= n_packets; TIME_OVERFLOW: the set of records of the packets whose arrival reaches
    2^64 - 1 (the library names one of them); OK: None."""
    n = len(enter)
    assert bad_link_off(link_off, n) is None and len(base) == n_packets
    ent, wt, dn = ([int(x) for x in np.asarray(a).tolist()] for a in (enter, wait, done))
    pk = [int(x) for x in np.asarray(packet).tolist()]
    for i in range(n):
        if pk[i] >= n_packets:
            return INVALID_ARG, i, None, None, None
    recs = [[] for _ in range(n_packets)]
    for i in range(n):
        recs[pk[i]].append(i)
    delay, arrive, where = [0] * n_packets, [0] * n_packets, [NOTHING] * n_packets
    over = set()
    for p in range(n_packets):
        b = int(base[p])
        arrive[p] = b
        if not recs[p]:
            continue
        dropped = [i for i in recs[p] if state(wt[i], dn[i]) == "dropped"]
        t_drop = None
        if dropped:
            d = min(dropped, key=lambda i: (ent[i], i))
            where[p], t_drop = d, ent[d]
        else:
            where[p] = ARRIVED
        counted = [i for i in recs[p] if state(wt[i], dn[i]) == "served" and (t_drop is None or ent[i] < t_drop)]
        if counted:
            if carry:
                last = max(counted, key=lambda i: ent[i])
                delay[p] = dn[last] - ent[last]
            else:
                delay[p] = sum(dn[i] - ent[i] for i in counted) & MAX
        if dropped:
            arrive[p] = MAX
        else:
            arrive[p] = min(b + delay[p], MAX)
            if arrive[p] == MAX:
                over.update(recs[p])
    if over:
        return TIME_OVERFLOW, over, None, None, None
    return OK, None, np.array(delay, np.uint64), np.array(arrive, np.uint64), np.array(where, np.uint32)


def check_args(n_records, packet, wait, done, ahead):
    """The errors that leave every output untouched, in the library's order after the call's own."""
    if packet is None or wait is None or done is None or ahead is None:
        return INVALID_ARG
    return CAPACITY if n_records > (1 << 32) - 2 else OK
