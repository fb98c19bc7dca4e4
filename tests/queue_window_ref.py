"""Windowed link queues (sg_link_queue with its window flag), the definition restated over Python
integers (include/shadow_gpu.h, "link queues"), built on queue_carry_ref.event
and queue_drop_ref.event.

  * `define`: the closed solution (the carried call without the bit), the classification against
    the horizon H, the re-based enter times r of the pending records and the packet tails.
  * `jacobi`: the loop the library runs, restated: a compact view of the records whose carried time is
    below H, sorted and scanned per iteration; it counts its iterations and the records it sorted,
    and asserts the two invariants and the iteration bound as it goes.
  * `SessionRef`: rounds that queue behind one another, by re-feeding: what shadow_amd.LinkQueueSession
    keeps, over any `solve` that answers one windowed call (define here, the library on the card).

A case is a queue_carry_cases.case dict, with limit_ns under the drop rule and base with packets.
define and jacobi return a dict: the call's eight arrays by queue_ref.FIELDS name (busy and
ahead_max doubled under the drop rule, the packet tails behind the records with packets), plus
"pending" (bool per record), "lost", and for jacobi "iters" and "active".
"""
import numpy as np

import outcomes_ref as OR
import queue_carry_ref as CR
import queue_drop_ref as DR
import queue_ref as QR
from queue_ref import MAX, OK, TIME_OVERFLOW, UMAX

WINDOW_FLAG = "SG_LINK_" + "QUEUE_WINDOW"  # (in two parts: queue_carry_cases.CARRY_FLAG tells why)
WINDOW = 0x20
IN_FLIGHT = 0xFFFFFFFD
NONE = CR.NO_NEXT


def _closed(c, drop):
    if drop:
        return DR.event(c["link_off"], c["enter"], c["packet"], c["weight"], n_packets=c["n_packets"], cost_ps=c["cost_ps"],
                        limit_ns=c["limit_ns"], free_in=c["free_in"])
    return CR.event(c["link_off"], c["enter"], c["packet"], c["weight"], n_packets=c["n_packets"], cost_ps=c["cost_ps"],
                    free_in=c["free_in"])


def _chains(c):
    nxt, gap, first, _ = CR.chains(c["enter"], c["packet"], c["n_packets"])
    prev = [NONE] * len(nxt)
    for i, k in enumerate(nxt):
        if k != NONE:
            prev[k] = i
    return nxt, prev, gap, first


def _links(c):
    off = np.asarray(c["link_off"]).astype(np.int64)
    return off, np.repeat(np.arange(len(off) - 1), np.diff(off)).tolist()


def _services(c, link):
    w = CR._weights(len(link), c["packet"], c["weight"])
    return [QR.service(w[i], c["cost_ps"][link[i]]) for i in range(len(link))]


def _finish(c, drop, packets, state, wait, done, ahead, rebased):
    """The outputs from every record's state ("served", "dropped", "absent", "pending"), the settled
    records' values and the pending records' re-based times."""
    off, link = _links(c)
    nl, n = len(off) - 1, len(link)
    s = _services(c, link)
    free = [0 if c["free_in"] is None else int(c["free_in"][k]) for k in range(nl)]
    w_out, d_out, a_out = [MAX] * n, [MAX] * n, [0] * n
    for i in range(n):
        if state[i] == "pending":
            if rebased[i] >= MAX:
                return TIME_OVERFLOW
            d_out[i], a_out[i] = rebased[i], UMAX
        elif state[i] == "served":
            w_out[i], d_out[i], a_out[i] = wait[i], done[i], ahead[i]
            free[link[i]] = max(free[link[i]], done[i])  # (a link's done never falls)
        elif state[i] == "dropped":
            d_out[i], a_out[i] = done[i], ahead[i]
    sums = DR._link_sums(nl, link, state, s, w_out, a_out)
    busy, wmax, wsum, amax, drops, refused = sums
    out = dict(wait=np.array(w_out, np.uint64), done=np.array(d_out, np.uint64), ahead=np.array(a_out, np.uint32),
               link_free=np.array(free, np.uint64), busy=np.array(busy + (refused if drop else []), np.uint64),
               wait_max=np.array(wmax, np.uint64), wait_sum=np.array(wsum, np.uint64),
               ahead_max=np.array(amax + (drops if drop else []), np.uint32),
               pending=np.array([x == "pending" for x in state], bool), lost=0)
    if not packets:
        return out
    P = c["n_packets"]
    ent = [int(x) for x in np.asarray(c["enter"]).tolist()]
    pk = np.asarray(c["packet"]).tolist()
    delay, arrive, where = [0] * P, [int(b) for b in c["base"]], [OR.NOTHING] * P
    recs = [[] for _ in range(P)]
    for i in range(n):
        recs[pk[i]].append(i)
    for p in range(P):
        if not recs[p]:
            continue
        recs[p].sort(key=lambda i: ent[i])
        where[p] = OR.ARRIVED
        for i in recs[p]:
            if state[i] == "served":
                delay[p] = done[i] - ent[i]
            elif state[i] == "dropped":
                where[p] = i
                break
            elif state[i] == "pending":
                where[p], delay[p] = IN_FLIGHT, rebased[i] - ent[i]
                break
        if where[p] < IN_FLIGHT:
            arrive[p] = MAX
            out["lost"] += 1
        else:
            arrive[p] = min(arrive[p] + delay[p], MAX)
            if arrive[p] == MAX:
                return TIME_OVERFLOW
    out["wait"] = np.concatenate([out["wait"], np.array(delay, np.uint64)])
    out["done"] = np.concatenate([out["done"], np.array(arrive, np.uint64)])
    out["ahead"] = np.concatenate([out["ahead"], np.array(where, np.uint32)])
    return out


def define(c, H, drop=False, packets=False):
    """The definition: (status, outputs).  The closed solution must succeed (an overflow past the
    horizon is not the windowed call's to find: no case has one)."""
    rc, pair, res, cur, _ = _closed(c, drop)
    if rc != OK:
        return rc, pair
    n = len(cur)
    nxt, prev, gap, first = _chains(c)
    e = [int(x) for x in cur.tolist()]  # (2^64 - 1: absent)
    closed_state = ["served"] * n
    if drop:
        srv, drp, _ = DR.states(res)
        closed_state = ["served" if srv[i] else "dropped" if drp[i] else "absent" for i in range(n)]
    state, rebased = [None] * n, [0] * n
    for h in range(n):
        if not first[h]:
            continue
        i, live = h, True  # live: no settled drop so far
        pend = False
        while i != NONE:
            if pend:
                state[i], rebased[i] = "pending", min(rebased[prev[i]] + gap[prev[i]], MAX)
            elif not live:
                state[i] = "absent"
            elif e[i] < H:
                state[i] = closed_state[i]
                assert state[i] != "absent"
                live = state[i] == "served"
            else:
                # the first pending record: its chain's first, or behind a settled served record
                pend, state[i] = True, "pending"
                rebased[i] = int(c["enter"][i]) if first[i] else e[i]
                assert first[i] or (closed_state[prev[i]] == "served" and e[i] == int(res.done[prev[i]]) + gap[prev[i]])
            i = nxt[i]
    out = _finish(c, drop, packets, state, res.wait.tolist(), res.done.tolist(), res.ahead.tolist(), rebased)
    return (TIME_OVERFLOW, None) if isinstance(out, int) else (OK, out)


def iteration_bound(c, H):
    """ceil((H - t_min) / g_min) + 1 with t_min the smallest enter below H and g_min the smallest gap:
    the + 1 is the pass that sees nothing move.  1 when no record is below H; 2 when there is no gap
    (single records: nothing can move)."""
    ent = [int(x) for x in np.asarray(c["enter"]).tolist()]
    below = [t for t in ent if t < H]
    if not below:
        return 1
    nxt, _, gap, _ = _chains(c)
    gaps = [gap[i] for i in range(len(ent)) if nxt[i] != NONE]
    if not gaps:
        return 2
    return -((min(below) - H) // min(gaps)) + 1


def jacobi(c, H, drop=False, packets=False, exact=None, cap=4096):
    """The library's loop: (status, outputs with "iters" and "active").  exact: the closed solution's
    carried enter times, to assert the first invariant against."""
    off, link = _links(c)
    nl, n = len(off) - 1, len(link)
    nxt, prev, gap, first = _chains(c)
    pk = np.asarray(c["packet"], np.uint32)
    cur = [int(x) for x in np.asarray(c["enter"]).tolist()]
    below = [t for t in cur if t < H]
    gaps = [gap[i] for i in range(n) if nxt[i] != NONE]
    t_min, g_min = (min(below) if below else None), (min(gaps) if gaps else None)

    def compact():
        """The marks over the times as they stand, then the stale records' new times."""
        act = [cur[i] < H and (prev[i] == NONE or cur[prev[i]] < H) for i in range(n)]
        moved = False
        for i in range(n):
            if not act[i] and cur[i] < H:
                assert cur[prev[i]] >= H  # (its predecessor is not written here)
                cur[i], moved = min(cur[prev[i]] + gap[prev[i]], MAX), True
        return [i for i in range(n) if act[i]], moved

    def stale():
        return {i for i in range(n) if prev[i] != NONE and cur[prev[i]] >= H and cur[i] < H}

    view, moved = compact()
    assert not moved
    iters = active = 0
    behind = set()
    while True:
        if iters == cap:
            return CR.CAPACITY, None
        iters += 1
        active += len(view)
        changed = False
        res = perm = None
        if view:
            by = [[] for _ in range(nl)]
            for i in view:
                by[link[i]].append(i)
            perm = [i for k in range(nl) for i in sorted(by[k], key=lambda i: (cur[i], int(pk[i])))]
            coff = np.cumsum([0] + [len(b) for b in by]).astype(np.uint64)
            p_arr = np.array(perm, np.int64)
            ent = np.array([cur[i] for i in perm], np.uint64)
            if drop:
                rc, _, res = DR.loop(coff, ent, pk[p_arr], c["weight"], cost_ps=c["cost_ps"], limit_ns=c["limit_ns"],
                                     free_in=c["free_in"])
            else:
                rc, _, res = QR.loop(coff, ent, pk[p_arr], c["weight"], cost_ps=c["cost_ps"], free_in=c["free_in"])
            if rc == TIME_OVERFLOW:
                return TIME_OVERFLOW, None
            assert rc == OK
            done, wait = res.done.tolist(), res.wait.tolist()
            for j, i in enumerate(perm):
                if nxt[i] != NONE:
                    v = MAX
                    if wait[j] != MAX:
                        v = min(done[j] + gap[i], MAX)
                        if v == MAX:
                            return TIME_OVERFLOW, None
                    if v != cur[nxt[i]]:
                        cur[nxt[i]], changed = v, True
        nview, moved = compact()
        # invariant 2: what stood behind a record that left the window is rewritten an iteration later
        assert all(cur[i] >= H for i in behind)
        behind = stale()
        # invariant 1: an estimate that is not exact is not below t_min + iterations x g_min
        if exact is not None and t_min is not None and g_min is not None:
            for i in range(n):
                ok = cur[i] == int(exact[i]) or (int(exact[i]) >= H and cur[i] >= H)
                assert ok or cur[i] >= t_min + iters * g_min, (i, cur[i], int(exact[i]), iters)
        if not (changed or moved):
            break
        view = nview
    assert not behind and nview == view
    state, rebased = ["absent"] * n, [0] * n
    wait, done, ahead = [MAX] * n, [MAX] * n, [0] * n
    if view:
        for j, i in enumerate(perm):
            wait[i], done[i], ahead[i] = int(res.wait[j]), int(res.done[j]), int(res.ahead[j])
            state[i] = "served" if wait[i] != MAX else "dropped"

    def tail(k, r, absent):
        while k != NONE:
            state[k], rebased[k] = ("absent" if absent else "pending"), r
            r, k = min(r + gap[k], MAX), nxt[k]

    for i in view:
        if nxt[i] != NONE and cur[nxt[i]] >= H:
            tail(nxt[i], cur[nxt[i]], state[i] == "dropped")
    for i in range(n):
        if first[i] and cur[i] >= H:
            tail(i, cur[i], False)
    out = _finish(c, drop, packets, state, wait, done, ahead, rebased)
    if isinstance(out, int):
        return TIME_OVERFLOW, None
    out["iters"], out["active"] = iters, active
    return OK, out


def pending_mask(wait, ahead, n):
    return (np.asarray(wait[:n]) == np.uint64(MAX)) & (np.asarray(ahead[:n]) == np.uint32(UMAX))


class SessionRef:
    """Rounds that queue behind one another.  solve(case, H, drop) -> a windowed call's outputs with
    packets (define's dict).  advance() takes a round's case (its own packet numbers, base, weight)
    and returns the settled records [(round, record, wait, done)] and the settled packets
    [(round, packet, delay against the original base, arrive, where's link or None, lost)]."""

    def __init__(self, n_links, cost_ps, limit_ns=None, free_in=None, solve=None):
        self.nl, self.cost, self.limit = n_links, np.asarray(cost_ps, np.uint64), limit_ns
        self.free = np.zeros(n_links, np.uint64) if free_in is None else np.asarray(free_in, np.uint64).copy()
        self.solve = solve or (lambda c, H, drop: define(c, H, drop, True)[1])
        self.rec = []  # pending records: (link, re-based enter, in-flight slot, (round, record))
        self.pkt = []  # in-flight packets: (weight, re-based base, original base, (round, packet))
        self.last, self.round = 0, 0
        self.sums = dict(busy=np.zeros(n_links, np.uint64), wait_sum=np.zeros(n_links, np.uint64),
                         wait_max=np.zeros(n_links, np.uint64), drops=np.zeros(n_links, np.uint64))

    def advance(self, new, H):
        assert H >= self.last and (new is None or not len(new["enter"]) or int(new["enter"].min()) >= self.last)
        F, rnd, drop = len(self.pkt), self.round, self.limit is not None
        rows = list(self.rec)
        pkts = list(self.pkt)
        if new is not None:
            off = new["link_off"].astype(np.int64)
            for k in range(self.nl):
                rows += [(k, int(new["enter"][i]), F + int(new["packet"][i]), (rnd, i)) for i in range(off[k], off[k + 1])]
            pkts += [(int(new["weight"][p]), int(new["base"][p]), int(new["base"][p]), (rnd, p)) for p in range(new["n_packets"])]
        rows.sort(key=lambda r: r[0])  # (stable: pending before new on every link, each in its order)
        n, P = len(rows), len(pkts)
        link = np.array([r[0] for r in rows], np.int64)
        c = dict(link_off=np.searchsorted(link, np.arange(self.nl + 1)).astype(np.uint64),
                 enter=np.array([r[1] for r in rows], np.uint64), packet=np.array([r[2] for r in rows], np.uint32),
                 weight=np.array([p[0] for p in pkts], np.uint32), base=np.array([p[1] for p in pkts], np.uint64),
                 cost_ps=self.cost, free_in=self.free, n_packets=P)
        if drop:
            c["limit_ns"] = self.limit
        out = self.solve(c, H, drop)
        pend = pending_mask(out["wait"], out["ahead"], n)
        delay, arrive, where = out["wait"][n:], out["done"][n:], out["ahead"][n:]
        flying = where == np.uint32(IN_FLIGHT)
        slot = np.cumsum(flying) - 1
        records = [(rows[i][3][0], rows[i][3][1], int(out["wait"][i]), int(out["done"][i])) for i in range(n) if not pend[i]]
        packets = []
        for p in range(P):
            if not flying[p]:
                lost = int(where[p]) < IN_FLIGHT
                packets.append((pkts[p][3][0], pkts[p][3][1], (int(delay[p]) + pkts[p][1] - pkts[p][2]) & MAX, int(arrive[p]),
                                int(link[int(where[p])]) if lost else None, lost))
        self.rec = [(rows[i][0], int(out["done"][i]), int(slot[rows[i][2]]), rows[i][3]) for i in range(n) if pend[i]]
        self.pkt = [(pkts[p][0], int(arrive[p]), pkts[p][2], pkts[p][3]) for p in range(P) if flying[p]]
        assert all(flying[rows[i][2]] for i in range(n) if pend[i])
        self.free = out["link_free"].copy()
        self.sums["busy"] += out["busy"][:self.nl]
        self.sums["wait_sum"] += out["wait_sum"]
        self.sums["wait_max"] = np.maximum(self.sums["wait_max"], out["wait_max"])
        if drop:
            self.sums["drops"] += out["ahead_max"][self.nl:].astype(np.uint64)
        self.last, self.round = H, rnd + 1
        return records, packets

    def flush(self):
        return self.advance(None, MAX)
