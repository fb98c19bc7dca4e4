"""Link queues with finite buffers (sg_link_queue with its drop flag), the definition restated
(include/shadow_gpu.h, "link queues"), over Python integers.  Built beside
queue_ref.py and queue_carry_ref.py, whose input checks and chains it shares.

limit_ns[L] is the longest wait link L's buffer holds (2^64 - 1: no limit).  Per link, in the order
served, `done` starting at free_in[L]:
    start = max(enter, done)
    start - enter > limit_ns[L]: the record is dropped, done stays;  else it is served:
    done = min(start + s, 2^64 - 1), wait = start - enter
    ahead = #{earlier served records of the link's order with done > enter}

  * `loop`: first order, a plain loop per link, `ahead` by direct count.  Deliberately not the
    library's algorithm (an unlimited scan, busy periods walked from an idle server, a binary
    search over the running done).
  * `event`: carried, an event-driven simulation in global (time, packet) order: the successor of
    a dropped record never arrives.
  * `jacobi`: carried, the fixed point the library iterates, started from the trace's times with
    every record present; a successor that never arrives has the time 2^64 - 1, sorts last on its
    link and is skipped by `loop` (absent=True).

Per record the state is read from the sentinels: served (wait, done, ahead); dropped (2^64 - 1, its
(carried) enter time, the served records it found); absent (2^64 - 1, 2^64 - 1, 0).  Per link:
link_free (the done of the record served last, free_in when none was), busy, wait_max, wait_sum and
ahead_max over served records; drops (u32) and refused (the dropped records' summed service, wraps).
Only a served record overflows: its done, or carried its done + gap, reaching 2^64 - 1.
"""
import bisect
import heapq
from collections import namedtuple

import numpy as np

import queue_carry_ref as CR
import queue_ref as QR
from queue_ref import INVALID_ARG, MAX, OK, TIME_OVERFLOW, UMAX, bad_link_off, service  # noqa: F401

CAPACITY = CR.CAPACITY
NO_NEXT = CR.NO_NEXT
# The flag's name, in two parts (queue_carry_cases.CARRY_FLAG tells why).
DROP_FLAG = "SG_LINK_" + "QUEUE_DROP"

Result = namedtuple("Result", QR.FIELDS + ("drops", "refused"))
FIELDS = Result._fields
RECORD_FIELDS = QR.RECORD_FIELDS
DTYPES = dict(QR.DTYPES, drops=np.uint32, refused=np.uint64)


def states(res):
    """(served, dropped, absent) per record, from the sentinels."""
    out = res.wait == np.uint64(MAX)
    absent = out & (res.done == np.uint64(MAX))
    return ~out, out & ~absent, absent


def _link_sums(nl, link, state, s, wait, ahead):
    busy, wmax, wsum, amax, drops, refused = ([0] * nl for _ in range(6))
    for i, lk in enumerate(link):
        if state[i] == "served":
            busy[lk] = (busy[lk] + s[i]) & MAX
            wsum[lk] = (wsum[lk] + wait[i]) & MAX
            wmax[lk] = max(wmax[lk], wait[i])
            amax[lk] = max(amax[lk], ahead[i])
        elif state[i] == "dropped":
            drops[lk] += 1
            refused[lk] = (refused[lk] + s[i]) & MAX
    return busy, wmax, wsum, amax, drops, refused


def _result(nl, link, state, s, wait, done, ahead, link_free):
    u = lambda x: np.array(x, np.uint64)  # noqa: E731
    busy, wmax, wsum, amax, drops, refused = _link_sums(nl, link, state, s, wait, ahead)
    return Result(u(wait), u(done), np.array(ahead, np.uint32), u(link_free), u(busy), u(wmax), u(wsum),
                  np.array(amax, np.uint32), np.array(drops, np.uint32), u(refused))


def loop(link_off, enter, packet=None, weight=None, *, cost_ps, limit_ns, free_in=None, absent=False, trace=None):
    """(status, (link, record in the link) or None, Result): first order, a segment at a time.
    absent: a record whose enter time is 2^64 - 1 is absent (the carried fixed point's use).
    trace: a list that receives the `done` after every record (the properties' tests)."""
    n = len(enter)
    bad = bad_link_off(link_off, n)
    if bad is not None:
        return INVALID_ARG, (bad, UMAX), None
    off = np.asarray(link_off).astype(np.int64)
    nl = len(off) - 1
    ent = [int(x) for x in np.asarray(enter).tolist()]
    w, bad_packet = QR.weights(n, packet, weight)
    link = np.repeat(np.arange(nl), np.diff(off)).tolist()
    s, wait, done, ahead, state = [0] * n, [MAX] * n, [MAX] * n, [0] * n, ["absent"] * n
    link_free = [0] * nl
    overflow = None
    for lk in range(nl):
        d = 0 if free_in is None else int(free_in[lk])
        lim = int(limit_ns[lk])
        seen = np.zeros(max(int(off[lk + 1] - off[lk]), 1), np.uint64)  # the done of the records served so far
        k = 0
        for i in range(int(off[lk]), int(off[lk + 1])):
            s[i] = service(w[i], cost_ps[lk])
            if not (absent and ent[i] == MAX):
                start = max(ent[i], d)
                ahead[i] = int((seen[:k] > np.uint64(ent[i])).sum())
                if start - ent[i] > lim:
                    state[i], done[i] = "dropped", ent[i]
                else:
                    d = min(start + s[i], MAX)
                    if d == MAX and overflow is None:
                        overflow = i
                    state[i], wait[i], done[i] = "served", start - ent[i], d
                    seen[k] = d
                    k += 1
            if trace is not None:
                trace.append(d)
        link_free[lk] = d
    res = _result(nl, link, state, s, wait, done, ahead, link_free)
    for code, i in ((INVALID_ARG, bad_packet), (TIME_OVERFLOW, overflow)):
        if i is not None:
            lk = int(np.searchsorted(off, i, side="right")) - 1
            return code, (lk, i - int(off[lk])), res
    return OK, None, res


def event(link_off, enter, packet, weight=None, *, n_packets, cost_ps, limit_ns, free_in=None):
    """(status, pair, Result, carried enter, None): the event-driven simulation."""
    n = len(enter)
    err, link = CR._check(link_off, enter, packet, n_packets)
    if err:
        return err[0], err[1], None, None, None
    off = np.asarray(link_off).astype(np.int64)
    nl = len(off) - 1
    pk = np.asarray(packet).tolist()
    w = CR._weights(n, packet, weight)
    nxt, gap, first, _ = CR.chains(enter, packet, n_packets)
    s = [service(w[i], cost_ps[link[i]]) for i in range(n)]
    done_l = [0 if free_in is None else int(free_in[k]) for k in range(nl)]
    served = [[] for _ in range(nl)]
    heap = [(int(enter[i]), pk[i], i) for i in range(n) if first[i]]
    heapq.heapify(heap)
    cur, wait, done, ahead, state = [MAX] * n, [MAX] * n, [MAX] * n, [0] * n, ["absent"] * n
    overflow = False
    while heap:
        t, _, i = heapq.heappop(heap)
        lk = link[i]
        start = max(t, done_l[lk])
        cur[i] = t
        ahead[i] = len(served[lk]) - bisect.bisect_right(served[lk], t)  # (the done times never fall)
        if start - t > int(limit_ns[lk]):
            state[i], done[i] = "dropped", t
            continue  # (its successor never arrives)
        d = min(start + s[i], MAX)
        overflow |= d == MAX
        state[i], wait[i], done[i] = "served", start - t, d
        served[lk].append(d)
        done_l[lk] = d
        if nxt[i] != NO_NEXT:
            v = min(d + gap[i], MAX)
            overflow |= v == MAX
            heapq.heappush(heap, (v, pk[nxt[i]], nxt[i]))
    if overflow:
        return TIME_OVERFLOW, None, None, None, None
    return OK, None, _result(nl, link, state, s, wait, done, ahead, done_l), np.array(cur, np.uint64), None


def jacobi(link_off, enter, packet, weight=None, *, n_packets, cost_ps, limit_ns, free_in=None, cap=4096):
    """(status, pair, Result, carried enter, iterations): the fixed point on `loop`."""
    n = len(enter)
    err, _ = CR._check(link_off, enter, packet, n_packets)
    if err:
        return err[0], err[1], None, None, 0
    off = np.asarray(link_off).astype(np.int64)
    pk = np.asarray(packet, np.uint32)
    nxt, gap, _, _ = CR.chains(enter, packet, n_packets)
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
        rc, _, res = loop(link_off, np.array([cur[i] for i in perm], np.uint64), pk[perm], weight, cost_ps=cost_ps,
                          limit_ns=limit_ns, free_in=free_in, absent=True)
        if rc == TIME_OVERFLOW:
            return TIME_OVERFLOW, None, None, None, iters
        assert rc == OK
        done, wait = res.done.tolist(), res.wait.tolist()
        changed = False
        for j, i in enumerate(perm.tolist()):
            if nxt[i] != NO_NEXT:
                v = MAX
                if wait[j] != MAX:  # served
                    v = min(done[j] + gap[i], MAX)
                    if v == MAX:
                        return TIME_OVERFLOW, None, None, None, iters
                if v != cur[nxt[i]]:
                    cur[nxt[i]], changed = v, True
        if not changed:
            break
    back = {k: np.empty_like(getattr(res, k)) for k in RECORD_FIELDS}
    for k in RECORD_FIELDS:
        back[k][perm] = getattr(res, k)
    return OK, None, res._replace(**back), np.array(cur, np.uint64), iters


def unlimited(nl):
    return np.full(nl, MAX, np.uint64)


def median_limits(link_off, wait):
    """The tests' and the benchmark's rule: limit_ns[L] is the median positive wait on L in an
    unlimited result (of an even count the two middle values' mean, rounded down), 2^64 - 1 on a
    link with no positive wait."""
    off = np.asarray(link_off).astype(np.int64)
    lim = unlimited(len(off) - 1)
    for lk in range(len(off) - 1):
        w = np.sort(wait[off[lk]:off[lk + 1]])
        w = w[w > 0]
        if len(w):
            lim[lk] = (int(w[(len(w) - 1) // 2]) + int(w[len(w) // 2])) // 2
    return lim
