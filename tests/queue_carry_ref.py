"""Carried link queues (sg_link_queue with its carry flag), the definition restated twice (include/shadow_gpu.h,
"link queues"), over Python integers.

  * `event`: an event-driven simulation.  A heap of arrivals (time, packet, record); the smallest
    is served on its link (start = max(time, the link's done), done = start + s) and the packet's
    next record arrives at done + gap.  Arrivals only ever lie in the future of the one at hand
    (gap >= 1), so the heap's order is the global (time, packet) order the definition names.
  * `jacobi`: the fixed point the library iterates, built on queue_ref.loop: sort every link's
    records by the carried times at hand, run the first-order loop over that order, move done +
    gap to each packet's next record, until no time moves.

A packet's chain is its records in ascending input enter; gap_i = enter[next(i)] - enter[i].
Both return (status, pair, Result, carried enter per record, iterations): Result is
queue_ref.Result with the per-record fields at the INPUT indices; iterations is None for `event`.
Errors, in this order: a bad link_off (INVALID_ARG, (link, UMAX)); packet[i] >= n_packets
(INVALID_ARG, (link, i - link_off[link]), the smallest i); two records of one packet at one time
(INVALID_ARG, the same kind of pair for the smallest record that has such a twin); done or done +
gap reaching 2^64 - 1 (TIME_OVERFLOW, pair None: unspecified); and for `jacobi` the iteration cap
(CAPACITY, (iterations, UMAX)).
"""
import bisect
import heapq

import numpy as np

import queue_ref as QR
from queue_ref import INVALID_ARG, MAX, OK, TIME_OVERFLOW, UMAX, Result, bad_link_off, service  # noqa: F401

CAPACITY = 10
NO_NEXT = -1


def _pair(off, i):
    lk = int(np.searchsorted(off, i, side="right")) - 1
    return lk, i - int(off[lk])


def chains(enter, packet, n_packets):
    """(next, gap, first, twin): next[i] (NO_NEXT for a chain's last record), gap[i], whether i is
    its chain's first record, and the smallest record with an equal-time twin in its chain (None)."""
    n = len(enter)
    ent = [int(x) for x in np.asarray(enter).tolist()]
    pk = np.asarray(packet).tolist()
    by = {}
    for i in range(n):
        by.setdefault(pk[i], []).append(i)
    nxt, gap, first, twin = [NO_NEXT] * n, [0] * n, [False] * n, None
    for recs in by.values():
        recs.sort(key=lambda i: (ent[i], i))
        first[recs[0]] = True
        for a, b in zip(recs, recs[1:]):
            nxt[a], gap[a] = b, ent[b] - ent[a]
            if gap[a] == 0:
                twin = a if twin is None else min(twin, a)
    return nxt, gap, first, twin


def _check(link_off, enter, packet, n_packets):
    """The input errors, or None; and the link of every record."""
    n = len(enter)
    bad = bad_link_off(link_off, n)
    if bad is not None:
        return (INVALID_ARG, (bad, UMAX)), None
    off = np.asarray(link_off).astype(np.int64)
    pk = np.asarray(packet).tolist()
    for i in range(n):
        if pk[i] >= n_packets:
            return (INVALID_ARG, _pair(off, i)), None
    twin = chains(enter, packet, n_packets)[3]
    if twin is not None:
        return (INVALID_ARG, _pair(off, twin)), None
    return None, np.repeat(np.arange(len(off) - 1), np.diff(off)).tolist()


def _weights(n, packet, weight):
    return [1] * n if weight is None else [int(weight[p]) for p in np.asarray(packet).tolist()]


def event(link_off, enter, packet, weight=None, *, n_packets, cost_ps, free_in=None):
    """The event-driven simulation."""
    n = len(enter)
    err, link = _check(link_off, enter, packet, n_packets)
    if err:
        return err[0], err[1], None, None, None
    off = np.asarray(link_off).astype(np.int64)
    nl = len(off) - 1
    pk = np.asarray(packet).tolist()
    w = _weights(n, packet, weight)
    nxt, gap, first, _ = chains(enter, packet, n_packets)
    s = [service(w[i], cost_ps[link[i]]) for i in range(n)]
    free = [0 if free_in is None else int(free_in[k]) for k in range(nl)]
    done_l = list(free)
    served = [[] for _ in range(nl)]  # the done times of a link's served records: they never fall
    heap = [(int(enter[i]), pk[i], i) for i in range(n) if first[i]]
    heapq.heapify(heap)
    cur, wait, done, ahead = [0] * n, [0] * n, [0] * n, [0] * n
    last = [None] * nl
    overflow = False
    while heap:
        t, _, i = heapq.heappop(heap)
        lk = link[i]
        start = max(t, done_l[lk])
        d = min(start + s[i], MAX)
        overflow |= d == MAX
        cur[i], wait[i], done[i] = t, start - t, d
        ahead[i] = len(served[lk]) - bisect.bisect_right(served[lk], t)
        served[lk].append(d)
        done_l[lk], last[lk] = d, i
        if nxt[i] != NO_NEXT:
            v = min(d + gap[i], MAX)
            overflow |= v == MAX
            heapq.heappush(heap, (v, pk[nxt[i]], nxt[i]))
    if overflow:
        return TIME_OVERFLOW, None, None, None, None
    res = _result(off, link, s, wait, done, ahead, free_in, [free[k] if last[k] is None else done[last[k]] for k in range(nl)])
    return OK, None, res, np.array(cur, np.uint64), None


def _result(off, link, s, wait, done, ahead, free_in, link_free):
    nl = len(off) - 1
    u = lambda x: np.array(x, np.uint64)  # noqa: E731
    busy, wmax, wsum, amax = [0] * nl, [0] * nl, [0] * nl, [0] * nl
    for i, lk in enumerate(link):
        busy[lk] = (busy[lk] + s[i]) & MAX
        wsum[lk] = (wsum[lk] + wait[i]) & MAX
        wmax[lk] = max(wmax[lk], wait[i])
        amax[lk] = max(amax[lk], ahead[i])
    return Result(u(wait), u(done), np.array(ahead, np.uint32), u(link_free), u(busy), u(wmax), u(wsum), np.array(amax, np.uint32))


def jacobi(link_off, enter, packet, weight=None, *, n_packets, cost_ps, free_in=None, cap=4096):
    """The fixed point on queue_ref.loop."""
    n = len(enter)
    err, link = _check(link_off, enter, packet, n_packets)
    if err:
        return err[0], err[1], None, None, 0
    off = np.asarray(link_off).astype(np.int64)
    pk = np.asarray(packet, np.uint32)
    nxt, gap, _, _ = chains(enter, packet, n_packets)
    cur = [int(x) for x in np.asarray(enter).tolist()]
    iters = 0
    while True:
        if iters == cap:
            return CAPACITY, (iters, UMAX), None, None, iters
        iters += 1
        perm = []
        for k in range(len(off) - 1):
            perm += sorted(range(int(off[k]), int(off[k + 1])), key=lambda i: (cur[i], int(pk[i])))
        perm = np.array(perm, np.int64)
        rc, _, res = QR.loop(link_off, np.array([cur[i] for i in perm], np.uint64), pk[perm], weight, cost_ps=cost_ps,
                             free_in=free_in)
        if rc == TIME_OVERFLOW:
            return TIME_OVERFLOW, None, None, None, iters
        assert rc == OK
        done = res.done.tolist()
        changed = False
        for j, i in enumerate(perm.tolist()):
            if nxt[i] != NO_NEXT:
                v = min(done[j] + gap[i], MAX)
                if v == MAX:
                    return TIME_OVERFLOW, None, None, None, iters
                if v != cur[nxt[i]]:
                    cur[nxt[i]], changed = v, True
        if not changed:
            break
    back = {k: np.empty_like(getattr(res, k)) for k in QR.RECORD_FIELDS}
    for k in QR.RECORD_FIELDS:
        back[k][perm] = getattr(res, k)
    return OK, None, res._replace(**back), np.array(cur, np.uint64), iters


def order_changes(link_off, enter, cur, packet):
    """Whether some link's service order (ascending (carried enter, packet)) is not its input order."""
    off = np.asarray(link_off).astype(np.int64)
    pk = np.asarray(packet).tolist()
    c = np.asarray(cur).tolist()
    for k in range(len(off) - 1):
        seg = list(range(int(off[k]), int(off[k + 1])))
        if sorted(seg, key=lambda i: (c[i], pk[i])) != seg:
            return True
    return False
